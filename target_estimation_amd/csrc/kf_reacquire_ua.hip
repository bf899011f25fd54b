// kf_reacquire_ua.hip -- the uniform_acceleration instances of reacquire_kernel (kf_reacquire_impl.hpp), one per Ops table entry of
// kf_model_ua.hip / kf_shared_ua.hip: a translation unit of its own so that the build stays parallel.
#include "kf_reacquire_impl.hpp"

namespace te {

TE_REACQUIRE_COMMON(ModelUA)
TE_REACQUIRE_INSTANCE(ModelUA, double, 1, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelUA, double, 1, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelUA, float, 1, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelUA, float, 1, LAYOUT_PACKED)

}  // namespace te
