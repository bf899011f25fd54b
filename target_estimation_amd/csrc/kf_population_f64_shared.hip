// kf_population_f64_shared.hip -- the one-launch population tick in fp64 for managers whose batches are all in the shared-axes
// storage form (kf_step_population_kernel<T, SHARED = true, VAR>): a translation unit of its own so that the build
// stays parallel.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_step_f64_shared(const StepParams parts[4], bool query, bool ab, bool reverse, hipStream_t s) {
  launch_population_step_t<double, true>(parts, query, ab, reverse, s);
}

}  // namespace te
