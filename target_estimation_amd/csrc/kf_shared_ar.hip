// kf_shared_ar.hip -- the kernels of one motion model for batches in the shared-axes storage form (te_layout.hpp
// LAYOUT_SEPARABLE_SHARED; fp64, single-tick launches only): a translation unit of its own so that the build stays parallel.
#include "kf_ops_impl.hpp"

namespace te {

const Ops* get_ops_shared_ar() { return OpsImpl<ModelAR, double, 1, LAYOUT_SEPARABLE_SHARED>::get(); }

}  // namespace te
