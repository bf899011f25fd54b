// kf_gate_impl.hpp -- included by kf_gate_{uv,ua,ar,av}.hip: the gated single-tick step kernels (kf_step_sep.hpp,
// kf_step_sep_gate_kernel: the kInnov tick in two phases around the NIS gate), one motion model per translation unit -- the
// axis-separable layout and the one with packed groups in fp64 and fp32, and the shared-axes storage form in fp64.
// OpsImpl::step (kf_ops_impl.hpp) launches them through launch_sep_gate_step.
#pragma once
#include "kf_ops_impl.hpp"

namespace te {

template <class M, typename T, int LAYOUT>
void launch_sep_gate_step(const StepArgs<T>& a, double gate, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_gate_kernel<M, T, LAYOUT>), dim3(blocks), dim3(threads), 0, s, a, gate);
}

#define TE_GATE_INSTANCES(M)                                                                                                         \
  template void launch_sep_gate_step<M, double, LAYOUT_SEPARABLE>(const StepArgs<double>&, double, unsigned, unsigned, hipStream_t);        \
  template void launch_sep_gate_step<M, double, LAYOUT_SEPARABLE_PACKED>(const StepArgs<double>&, double, unsigned, unsigned, hipStream_t); \
  template void launch_sep_gate_step<M, double, LAYOUT_SEPARABLE_SHARED>(const StepArgs<double>&, double, unsigned, unsigned, hipStream_t); \
  template void launch_sep_gate_step<M, float, LAYOUT_SEPARABLE>(const StepArgs<float>&, double, unsigned, unsigned, hipStream_t);          \
  template void launch_sep_gate_step<M, float, LAYOUT_SEPARABLE_PACKED>(const StepArgs<float>&, double, unsigned, unsigned, hipStream_t);

}  // namespace te
