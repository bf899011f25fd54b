// kf_population_fused_f32.hip -- one instantiation of the one-launch fused replay of a whole population (kf_population_fused_impl.hpp,
// kf_step_population_fused_kernel<float, GATE false, DTTAB false>): a translation unit of its own so that the build stays parallel.
#include "kf_population_fused_impl.hpp"

namespace te {

TE_POPULATION_FUSED_UNIT(float, false, false)

}  // namespace te
