// kf_population_f64_shared_pose.hip -- the shared-axes population tick (kf_population_f64_shared.hip) with the per-tick pose stream.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_grid_pose_shared(const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, bool query, bool ab, hipStream_t s) {
  launch_population_grid<double, true, true>(p, blocks, wpb, query, ab, s);
}

}  // namespace te
