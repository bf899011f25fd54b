// kf_reacquire_av.hip -- the angular_velocities instances of reacquire_kernel (kf_reacquire_impl.hpp), one per Ops table entry of
// kf_model_av.hip / kf_model_av_sym.hip / kf_shared_av.hip: a translation unit of its own so that the build stays parallel.
#include "kf_reacquire_impl.hpp"

namespace te {

TE_REACQUIRE_COMMON(ModelAV)
TE_REACQUIRE_INSTANCE(ModelAV, double, 6, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelAV, double, 1, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelAV, double, 6, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelAV, float, 1, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelAV, float, 6, LAYOUT_FULL)
TE_REACQUIRE_INSTANCE(ModelAV, float, 1, LAYOUT_PACKED)
TE_REACQUIRE_INSTANCE(ModelAV, float, 6, LAYOUT_PACKED)

}  // namespace te
