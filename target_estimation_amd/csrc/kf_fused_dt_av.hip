// kf_fused_dt_av.hip -- the angular_velocities temporally fused kernels with a time-step schedule, plain and gated (kf_fused_dt_impl.hpp): a
// translation unit of its own so that the build stays parallel and no existing object gains an instantiation.
#include "kf_fused_dt_impl.hpp"

namespace te {

TE_FUSED_DT_INSTANCES(ModelAV)

}  // namespace te
