// kf_population_impl.hpp -- included by kf_population_f64.hip / kf_population_f32.hip (one precision per translation unit: the
// kernel holds the step of all four motion models, a minute of compile time each).
#pragma once
#include "kf_ops_impl.hpp"
#include "kf_population.hpp"

namespace te {

// the grid of a population tick, POSE or not (the POSE variants are instantiated in kf_population_f{64,32}_pose.hip: one
// population translation unit already takes a minute to compile, so the pose stream's three kernels per precision get their own)
// SHARED: the parts are batches in the shared-axes storage form (fp64; kf_population_f64_shared{,_pose}.hip)
template <typename T, bool POSE, bool SHARED = false>
void launch_population_grid(const PopulationArgs<T>& p, unsigned blocks, unsigned wpb, bool query, bool ab, hipStream_t s) {
  const dim3 blk(64 * wpb);
  if (query) hipLaunchKernelGGL((kf_step_population_kernel<T, true, false, POSE, SHARED>), dim3(blocks), blk, 0, s, p);
  else if (ab) hipLaunchKernelGGL((kf_step_population_kernel<T, false, true, POSE, SHARED>), dim3(blocks), blk, 0, s, p);
  else hipLaunchKernelGGL((kf_step_population_kernel<T, false, false, POSE, SHARED>), dim3(blocks), blk, 0, s, p);
}
// the INNOV variant (in place, no fused query, no pose output): kf_population_f{64,32}_innov.hip, kf_population_f64_shared_innov.hip
template <typename T, bool SHARED>
void launch_population_grid_innov_t(const PopulationArgs<T>& p, unsigned blocks, unsigned wpb, hipStream_t s) {
  hipLaunchKernelGGL((kf_step_population_kernel<T, false, false, false, SHARED, true>), dim3(blocks), dim3(64 * wpb), 0, s, p);
}
void launch_population_grid_innov_shared(const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_innov(const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_innov(const PopulationArgs<float>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_pose_shared(const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, bool query, bool ab, hipStream_t s);
void launch_population_grid_pose(const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, bool query, bool ab, hipStream_t s);
void launch_population_grid_pose(const PopulationArgs<float>& p, unsigned blocks, unsigned wpb, bool query, bool ab, hipStream_t s);

template <typename T, bool SHARED = false>
void launch_population_step_t(const StepParams parts[4], bool query, bool ab, bool reverse, hipStream_t s) {
  constexpr int TPW = 64;   // thread per target in every separable layout
  PopulationArgs<T> p;
  long waves_max = 0;
  bool pose = false;   // some part writes the pose stream (StepParams::pose, one block: a population launch is one tick)
  bool innov = false;  // some part writes the innovation stream (StepParams::nis)
  for (int k = 0; k < 4; ++k) {
    const StepParams& q = parts[k];
    if (q.n > 0 && q.pose) pose = true;
    if (q.n > 0 && q.nis) innov = true;
    if (q.n > 0 && (q.idx || q.cls || q.n_ticks != 1 || q.live_posted || q.o_pose || (query && !q.q_delta) || (ab && !q.rec_out) || (query && ab)))
      throw std::runtime_error("target_estimation_amd: a population launch takes dense single ticks of one-class batches");
    waves_max = std::max(waves_max, (q.n + TPW - 1) / TPW);
  }
  static const long small_grid = [] { const char* e = std::getenv("TE_SMALL_GRID_WAVES"); return e ? std::atol(e) : 1024L; }();
  static const int nt_env = [] { const char* e = std::getenv("TE_NT_MEAS"); return e ? std::atoi(e) : -1; }();
  // (as for the single-batch launches: small, latency-bound grids spread one wavefront per workgroup over the CUs)
  const int wpb = waves_max <= small_grid ? 1 : 4;
  unsigned end = 0;
  for (int k = 0; k < 4; ++k) {
    StepParams q = parts[k];
    q.reverse = 0;   // the order is reversed for the whole grid (PopulationArgs::reverse_blocks)
    p.part[k] = make_step_args<T>(q);
    if (nt_env >= 0) p.part[k].nt_meas = nt_env;
    const long waves = (q.n + TPW - 1) / TPW;
    end += (unsigned)((waves + wpb - 1) / wpb);
    p.end[k] = end;
  }
  if (end == 0) return;
  p.reverse_blocks = reverse ? 1 : 0;
  if (innov) {
    if (query || ab || pose)
      throw std::runtime_error("target_estimation_amd: a population launch with an innovation stream is a plain tick in place (the query and the poses follow as launches of their own)");
    if constexpr (SHARED) launch_population_grid_innov_shared(p, end, (unsigned)wpb, s);
    else launch_population_grid_innov(p, end, (unsigned)wpb, s);
    return;
  }
  if constexpr (SHARED) {
    if (pose) launch_population_grid_pose_shared(p, end, (unsigned)wpb, query, ab, s);
    else launch_population_grid<T, false, true>(p, end, (unsigned)wpb, query, ab, s);
  } else {
    if (pose) launch_population_grid_pose(p, end, (unsigned)wpb, query, ab, s);
    else launch_population_grid<T, false>(p, end, (unsigned)wpb, query, ab, s);
  }
}

}  // namespace te
