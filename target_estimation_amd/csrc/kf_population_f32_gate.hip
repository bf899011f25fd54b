// kf_population_f32_gate.hip -- the one-launch population tick (float) with the NIS validation gate
// (kf_population_impl.hpp, kf_step_population_gate_kernel): a translation unit of its own so that the build stays parallel.
#include "kf_population_impl.hpp"

namespace te {

void launch_population_grid_gate(const PopulationArgs<float>& p, const PopulationGate& g, unsigned blocks, unsigned wpb, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_population_gate_kernel<float, false>), dim3(blocks), dim3(64 * wpb), 0, s, p, g);
}

}  // namespace te
