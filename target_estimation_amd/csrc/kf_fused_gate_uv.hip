// kf_fused_gate_uv.hip -- the uniform_velocity temporally fused kernels with the validation gate, the innovation stream and the re-acquisition
// policy inside the launched tick loop (kf_fused_gate_impl.hpp): a translation unit of its own so that the build stays parallel and no
// existing object gains an instantiation.
#include "kf_fused_gate_impl.hpp"

namespace te {

TE_FUSED_GATE_INSTANCES(ModelUV)

}  // namespace te
