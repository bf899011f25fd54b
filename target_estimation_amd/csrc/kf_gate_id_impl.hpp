// kf_gate_id_impl.hpp -- included by kf_gate_id_{uv,ua,ar,av}.hip: the gated by-id step kernels (kf_step_sep.hpp,
// kf_step_sep_gate_indexed_kernel: the gated kInnov | kIndexed tick with the update policy's tail), one motion model per
// translation unit -- the axis-separable layout and the one with packed groups in fp64 and fp32, and the shared-axes storage form
// in fp64.  OpsImpl::step (kf_ops_impl.hpp) launches them through launch_sep_gate_id_step.
#pragma once
#include "kf_ops_impl.hpp"

namespace te {

template <class M, typename T, int LAYOUT>
void launch_sep_gate_id_step(const StepArgs<T>& a, const GateById& g, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_gate_indexed_kernel<M, T, LAYOUT>), dim3(blocks), dim3(threads), 0, s, a, g);
}

#define TE_GATE_ID_INSTANCES(M)                                                                                                                     \
  template void launch_sep_gate_id_step<M, double, LAYOUT_SEPARABLE>(const StepArgs<double>&, const GateById&, unsigned, unsigned, hipStream_t);        \
  template void launch_sep_gate_id_step<M, double, LAYOUT_SEPARABLE_PACKED>(const StepArgs<double>&, const GateById&, unsigned, unsigned, hipStream_t); \
  template void launch_sep_gate_id_step<M, double, LAYOUT_SEPARABLE_SHARED>(const StepArgs<double>&, const GateById&, unsigned, unsigned, hipStream_t); \
  template void launch_sep_gate_id_step<M, float, LAYOUT_SEPARABLE>(const StepArgs<float>&, const GateById&, unsigned, unsigned, hipStream_t);          \
  template void launch_sep_gate_id_step<M, float, LAYOUT_SEPARABLE_PACKED>(const StepArgs<float>&, const GateById&, unsigned, unsigned, hipStream_t);

}  // namespace te
