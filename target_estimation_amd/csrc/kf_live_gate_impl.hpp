// kf_live_gate_impl.hpp -- included by kf_live_gate_{uv,ua,ar,av}.hip: the gated resident kernels (kf_step_sep.hpp,
// kf_step_sep_live_gate_kernel: the kFused | kLive2 tick loop with the two-phase gated body and the policy tail inside it), one
// motion model per translation unit -- the separable layout with packed groups, the one that has resident kernels, in fp64 and
// fp32.  OpsImpl::step (kf_ops_impl.hpp) launches them through launch_sep_live_gate_step; OpsImpl::live_capacity asks the
// occupancy query about them through live_gate_blocks_per_cu.
#pragma once
#include "kf_ops_impl.hpp"

namespace te {

template <class M, typename T, int LAYOUT>
void launch_sep_live_gate_step(const StepArgs<T>& a, const LiveGate& g, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_live_gate_kernel<M, T, LAYOUT>), dim3(blocks), dim3(threads), 0, s, a, g);
}

// one-wavefront workgroups of the kernel a CU holds at once (the occupancy query, static LDS included); 0 if the query fails
template <class M, typename T, int LAYOUT>
int live_gate_blocks_per_cu() {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kf_step_sep_live_gate_kernel<M, T, LAYOUT>, 64, 0) != hipSuccess) return 0;
  return per_cu;
}

#define TE_LIVE_GATE_INSTANCES(M)                                                                                                                    \
  template void launch_sep_live_gate_step<M, double, LAYOUT_SEPARABLE_PACKED>(const StepArgs<double>&, const LiveGate&, unsigned, unsigned, hipStream_t); \
  template void launch_sep_live_gate_step<M, float, LAYOUT_SEPARABLE_PACKED>(const StepArgs<float>&, const LiveGate&, unsigned, unsigned, hipStream_t);   \
  template int live_gate_blocks_per_cu<M, double, LAYOUT_SEPARABLE_PACKED>();                                                                            \
  template int live_gate_blocks_per_cu<M, float, LAYOUT_SEPARABLE_PACKED>();

}  // namespace te
