// kf_population_f64_shared_pose.hip -- the shared-axes population tick (kf_population_f64_shared.hip) with the per-tick pose stream.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_grid_pose_shared(unsigned v, const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s) {
  launch_population_grid<double, true, kPose, kQuery | kPose, kAB | kPose>(v, p, blocks, wpb, s);
}

}  // namespace te
