// kf_innov_impl.hpp -- included by kf_innov_{uv,ua,ar,av}.hip: the INNOV variants of the separable single-tick step kernel
// (kf_step_sep.hpp), one motion model per translation unit -- the axis-separable layout and the one with packed groups in fp64
// and fp32, and the shared-axes storage form in fp64.  OpsImpl::step (kf_ops_impl.hpp) launches them through
// launch_sep_innov_step.
#pragma once
#include "kf_ops_impl.hpp"

namespace te {

template <class M, typename T, int LAYOUT>
void launch_sep_innov_step(const StepArgs<T>& a, unsigned blocks, unsigned threads, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_sep_kernel<M, T, LAYOUT, kInnov>), dim3(blocks), dim3(threads), 0, s, a);
}

#define TE_INNOV_INSTANCES(M)                                                                                                  \
  template void launch_sep_innov_step<M, double, LAYOUT_SEPARABLE>(const StepArgs<double>&, unsigned, unsigned, hipStream_t);        \
  template void launch_sep_innov_step<M, double, LAYOUT_SEPARABLE_PACKED>(const StepArgs<double>&, unsigned, unsigned, hipStream_t); \
  template void launch_sep_innov_step<M, double, LAYOUT_SEPARABLE_SHARED>(const StepArgs<double>&, unsigned, unsigned, hipStream_t); \
  template void launch_sep_innov_step<M, float, LAYOUT_SEPARABLE>(const StepArgs<float>&, unsigned, unsigned, hipStream_t);          \
  template void launch_sep_innov_step<M, float, LAYOUT_SEPARABLE_PACKED>(const StepArgs<float>&, unsigned, unsigned, hipStream_t);

}  // namespace te
