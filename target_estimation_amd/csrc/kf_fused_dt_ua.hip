// kf_fused_dt_ua.hip -- the uniform_acceleration temporally fused kernels with a time-step schedule, plain and gated (kf_fused_dt_impl.hpp): a
// translation unit of its own so that the build stays parallel and no existing object gains an instantiation.
#include "kf_fused_dt_impl.hpp"

namespace te {

TE_FUSED_DT_INSTANCES(ModelUA)

}  // namespace te
