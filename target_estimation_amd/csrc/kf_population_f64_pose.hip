// kf_population_f64_pose.hip -- the one-launch population tick in fp64 with the per-tick pose stream (kf_population_impl.hpp,
// kf_step_population_kernel, the kPose variants): a translation unit of its own so that the build stays parallel.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_grid_pose(unsigned v, const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s) {
  launch_population_grid<double, false, kPose, kQuery | kPose, kAB | kPose>(v, p, blocks, wpb, s);
}

}  // namespace te
