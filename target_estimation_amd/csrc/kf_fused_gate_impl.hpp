// kf_fused_gate_impl.hpp -- included by kf_fused_gate_{uv,ua,ar,av}.hip: the launched temporally fused kernels with the validation
// gate, the innovation stream and the re-acquisition policy inside their tick loop (kf_step_sep.hpp, kf_step_sep_fused_gate_kernel:
// the kFused loop with the two-phase gated body and the policy tail), one motion model per translation unit -- the two separable
// layouts in fp64 and fp32.  OpsImpl::step (kf_ops_impl.hpp) launches them through launch_sep_fused_gate_step.
#pragma once
#include "kf_ops_impl.hpp"

namespace te {

template <class M, typename T, int LAYOUT>
void launch_sep_fused_gate_step(const StepArgs<T>& a, const FusedGate& g, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_fused_gate_kernel<M, T, LAYOUT>), dim3(blocks), dim3(threads), 0, s, a, g);
}

#define TE_FUSED_GATE_INSTANCE(M, T, LAYOUT) \
  template void launch_sep_fused_gate_step<M, T, LAYOUT>(const StepArgs<T>&, const FusedGate&, unsigned, unsigned, hipStream_t);
#define TE_FUSED_GATE_INSTANCES(M)                            \
  TE_FUSED_GATE_INSTANCE(M, double, LAYOUT_SEPARABLE)         \
  TE_FUSED_GATE_INSTANCE(M, double, LAYOUT_SEPARABLE_PACKED)  \
  TE_FUSED_GATE_INSTANCE(M, float, LAYOUT_SEPARABLE)          \
  TE_FUSED_GATE_INSTANCE(M, float, LAYOUT_SEPARABLE_PACKED)

}  // namespace te
