// kf_gate_id_ua.hip -- the uniform_acceleration by-id step kernels with the update policy (gate, rejection runs, re-initialisation:
// kf_gate_id_impl.hpp): a translation unit of its own so that the build stays parallel and no existing object gains an instantiation.
#include "kf_gate_id_impl.hpp"

namespace te {

TE_GATE_ID_INSTANCES(ModelUA)

}  // namespace te
