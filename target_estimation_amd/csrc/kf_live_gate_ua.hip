// kf_live_gate_ua.hip -- the uniform_acceleration resident kernels with the validation gate and the re-acquisition policy inside the session
// (kf_live_gate_impl.hpp): a translation unit of its own so that the build stays parallel and no existing object gains an instantiation.
#include "kf_live_gate_impl.hpp"

namespace te {

TE_LIVE_GATE_INSTANCES(ModelUA)

}  // namespace te
