// kf_reacquire_ar.hip -- the angular_rates instances of reacquire_kernel (kf_reacquire_impl.hpp), one per Ops table entry of
// kf_model_ar.hip / kf_shared_ar.hip: a translation unit of its own so that the build stays parallel.
#include "kf_reacquire_impl.hpp"

namespace te {

TE_REACQUIRE_COMMON(ModelAR)
TE_REACQUIRE_INSTANCE(ModelAR, double, 6, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelAR, double, 6, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelAR, float, 2, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelAR, float, 6, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelAR, float, 2, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelAR, float, 6, LAYOUT_PACKED)

}  // namespace te
