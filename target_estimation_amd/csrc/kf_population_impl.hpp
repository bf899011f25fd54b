// kf_population_impl.hpp -- included by kf_population_f64.hip / kf_population_f32.hip (one precision per translation unit: the
// kernel holds the step of all four motion models, a minute of compile time each).
#pragma once
#include "kf_ops_impl.hpp"
#include "kf_population.hpp"

namespace te {

// One launch of the population kernel of variant `v`, one of the V... this translation unit instantiates: the plain ticks
// (0, kQuery, kAB) with launch_population_step_t; the kPose variants in kf_population_f{64,32}_pose.hip and the kInnov one in
// kf_population_f{64,32}_innov.hip (one population translation unit already takes a minute to compile, so each stream's kernels
// get their own); SHARED -- the parts are batches in the shared-axes storage form, fp64 -- in kf_population_f64_shared{,_pose,_innov}.hip.
template <typename T, bool SHARED, unsigned... V>
void launch_population_grid(unsigned v, const PopulationArgs<T>& p, unsigned blocks, unsigned wpb, hipStream_t s) {
  const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * wpb), 0, s, p); return true; };
  if (!((v == V && launch(kf_step_population_kernel<T, SHARED, V>)) || ...)) throw std::runtime_error("target_estimation_amd: no population kernel for this request");
}
void launch_population_grid_innov_shared(unsigned v, const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_innov(unsigned v, const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_innov(unsigned v, const PopulationArgs<float>& p, unsigned blocks, unsigned wpb, hipStream_t s);
// the gated population tick (kf_step_population_gate_kernel), in kf_population_f{64,32}_gate.hip / kf_population_f64_shared_gate.hip
void launch_population_grid_gate_shared(const PopulationArgs<double>& p, const PopulationGate& g, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_gate(const PopulationArgs<double>& p, const PopulationGate& g, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_gate(const PopulationArgs<float>& p, const PopulationGate& g, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_pose_shared(unsigned v, const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_pose(unsigned v, const PopulationArgs<double>& p, unsigned blocks, unsigned wpb, hipStream_t s);
void launch_population_grid_pose(unsigned v, const PopulationArgs<float>& p, unsigned blocks, unsigned wpb, hipStream_t s);

template <typename T, bool SHARED = false>
void launch_population_step_t(const StepParams parts[4], bool query, bool ab, bool reverse, hipStream_t s) {
  constexpr int TPW = 64;   // thread per target in every separable layout
  PopulationArgs<T> p;
  long waves_max = 0;
  // the variant of the launch: the caller's query / ab, kPose / kInnov when some part writes that stream (StepParams::pose, one
  // block: a population launch is one tick; StepParams::nis)
  unsigned variant = (query ? kQuery : 0u) | (ab ? kAB : 0u);
  // a part with StepParams::gate set makes the launch the gated kernel: the kInnov tick with every part's gate (0: none)
  PopulationGate gates{{0.0, 0.0, 0.0, 0.0}};
  bool gated = false;
  for (int k = 0; k < 4; ++k) {
    const StepParams& q = parts[k];
    if (q.n <= 0) continue;
    const unsigned asked = requested_variant(q);
    if ((asked & ~(kQuery | kAB | kPose | kInnov)) || q.n_ticks != 1 || q.o_pose || (query && !q.q_delta) || (ab && !q.rec_out))
      throw std::runtime_error("target_estimation_amd: a population launch takes dense single ticks of one-class batches");
    variant |= asked & (kPose | kInnov);
    if (!(q.gate >= 0.0) || (q.gate > 0.0 && !q.nis))
      throw std::runtime_error("target_estimation_amd: the gate (nis_max) must be 0 (none) or positive, and needs the part's innovation stream");
    gates.gate[k] = q.gate;
    gated = gated || q.gate > 0.0;
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
  if (!population_variant_ok(variant, SHARED))
    throw std::runtime_error(sv_has(variant, kInnov)
                                 ? "target_estimation_amd: a population launch with an innovation stream is a plain tick in place (the query and the poses follow as launches of their own)"
                                 : "target_estimation_amd: a population launch takes dense single ticks of one-class batches");
  if (gated) {   // (variant == kInnov: population_variant_ok above)
    if constexpr (SHARED) launch_population_grid_gate_shared(p, gates, end, (unsigned)wpb, s);
    else launch_population_grid_gate(p, gates, end, (unsigned)wpb, s);
  } else if (sv_has(variant, kInnov)) {
    if constexpr (SHARED) launch_population_grid_innov_shared(variant, p, end, (unsigned)wpb, s);
    else launch_population_grid_innov(variant, p, end, (unsigned)wpb, s);
  } else if (sv_has(variant, kPose)) {
    if constexpr (SHARED) launch_population_grid_pose_shared(variant, p, end, (unsigned)wpb, s);
    else launch_population_grid_pose(variant, p, end, (unsigned)wpb, s);
  } else {
    launch_population_grid<T, SHARED, 0u, kQuery, kAB>(variant, p, end, (unsigned)wpb, s);
  }
}

}  // namespace te
