// kf_gate_ar.hip -- the angular_rates step kernels with the NIS validation gate (kf_gate_impl.hpp): a translation unit of its
// own so that the build stays parallel.
#include "kf_gate_impl.hpp"

namespace te {

TE_GATE_INSTANCES(ModelAR)

}  // namespace te
