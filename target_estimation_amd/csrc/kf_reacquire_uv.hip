// kf_reacquire_uv.hip -- the uniform_velocity instances of reacquire_kernel (kf_reacquire_impl.hpp), one per Ops table entry of
// kf_model_uv.hip / kf_shared_uv.hip: a translation unit of its own so that the build stays parallel.
#include "kf_reacquire_impl.hpp"

namespace te {

TE_REACQUIRE_COMMON(ModelUV)
TE_REACQUIRE_INSTANCE(ModelUV, double, 1, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelUV, double, 1, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelUV, float, 1, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelUV, float, 1, LAYOUT_PACKED)

}  // namespace te
