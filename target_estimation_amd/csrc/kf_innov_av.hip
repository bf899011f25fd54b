// kf_innov_av.hip -- the angular_velocities step kernels that also write the innovation stream (kf_innov_impl.hpp): a translation
// unit of its own so that the build stays parallel.
#include "kf_innov_impl.hpp"

namespace te {

TE_INNOV_INSTANCES(ModelAV)

}  // namespace te
