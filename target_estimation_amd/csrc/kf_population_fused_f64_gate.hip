// kf_population_fused_f64_gate.hip -- one instantiation of the one-launch fused replay of a whole population (kf_population_fused_impl.hpp,
// kf_step_population_fused_kernel<double, GATE true, DTTAB false>): a translation unit of its own so that the build stays parallel.
#include "kf_population_fused_impl.hpp"

namespace te {

TE_POPULATION_FUSED_UNIT(double, true, false)

}  // namespace te
