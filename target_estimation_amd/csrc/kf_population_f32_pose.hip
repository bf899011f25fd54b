// kf_population_f32_pose.hip -- the one-launch population tick in fp32 with the per-tick pose stream (kf_population_impl.hpp,
// kf_step_population_kernel<T, QUERY, AB, POSE = true>): a translation unit of its own so that the build stays parallel.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_grid_pose(const PopulationArgs<float>& p, unsigned blocks, unsigned wpb, bool query, bool ab, hipStream_t s) {
  launch_population_grid<float, true>(p, blocks, wpb, query, ab, s);
}

}  // namespace te
