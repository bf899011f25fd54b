// kf_fused_dt_impl.hpp -- included by kf_fused_dt_{uv,ua,ar,av}.hip: the launched temporally fused kernels with a time-step schedule
// (kf_step_sep.hpp, kf_step_sep_fused_dt_kernel and kf_step_sep_fused_gate_dt_kernel: the kFused loop, plain and gated, whose tick s
// runs with entry s of a device table), one motion model per translation unit -- the two separable layouts in fp64 and fp32.
// OpsImpl::step (kf_ops_impl.hpp) launches them through launch_sep_fused_dt_step / launch_sep_fused_gate_dt_step.
#pragma once
#include "kf_ops_impl.hpp"

namespace te {

template <class M, typename T, int LAYOUT>
void launch_sep_fused_dt_step(const StepArgs<T>& a, const double* dt_tab, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_fused_dt_kernel<M, T, LAYOUT>), dim3(blocks), dim3(threads), 0, s, a, dt_tab);
}
template <class M, typename T, int LAYOUT>
void launch_sep_fused_gate_dt_step(const StepArgs<T>& a, const FusedGate& g, const double* dt_tab, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_fused_gate_dt_kernel<M, T, LAYOUT>), dim3(blocks), dim3(threads), 0, s, a, g, dt_tab);
}

#define TE_FUSED_DT_INSTANCE(M, T, LAYOUT)                                                                                   \
  template void launch_sep_fused_dt_step<M, T, LAYOUT>(const StepArgs<T>&, const double*, unsigned, unsigned, hipStream_t); \
  template void launch_sep_fused_gate_dt_step<M, T, LAYOUT>(const StepArgs<T>&, const FusedGate&, const double*, unsigned, unsigned, hipStream_t);
#define TE_FUSED_DT_INSTANCES(M)                            \
  TE_FUSED_DT_INSTANCE(M, double, LAYOUT_SEPARABLE)         \
  TE_FUSED_DT_INSTANCE(M, double, LAYOUT_SEPARABLE_PACKED)  \
  TE_FUSED_DT_INSTANCE(M, float, LAYOUT_SEPARABLE)          \
  TE_FUSED_DT_INSTANCE(M, float, LAYOUT_SEPARABLE_PACKED)

}  // namespace te
