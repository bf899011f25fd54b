// kf_population_f32_innov.hip -- the one-launch population tick in fp32 with the per-tick innovation stream
// (kf_population_impl.hpp, kf_step_population_kernel, the kInnov variant): a translation unit of its own so that
// the build stays parallel.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_grid_innov(unsigned v, const PopulationArgs<float>& p, unsigned blocks, unsigned wpb, hipStream_t s) {
  launch_population_grid<float, false, kInnov>(v, p, blocks, wpb, s);
}

}  // namespace te
