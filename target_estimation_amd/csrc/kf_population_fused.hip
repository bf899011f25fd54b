// kf_population_fused.hip -- the launcher of the one-launch fused replay of a whole population (kf_population.hpp,
// launch_population_fused): host code only, the kernels live in kf_population_fused_f{64,32}{,_gate}{,_dt}.hip.
#include "kf_population_fused_impl.hpp"

namespace te {

template <typename T>
static void launch_population_fused_t(const StepParams parts[4], bool gated, const double* dt_tab, hipStream_t s) {
  constexpr int TPW = 64;   // thread per target in every separable layout
  const char* pre = "target_estimation_amd: a fused population launch: ";
  PopulationFusedArgs<T> p;
  long waves_max = 0;
  int n_ticks = 0;
  for (int k = 0; k < 4; ++k) {
    const StepParams& q = parts[k];
    if (q.n <= 0) continue;
    if (requested_variant(q) & ~(unsigned)kFused || q.n_ticks < 1 || q.o_pose || q.gate != 0.0 || q.reacq || q.gate_id || q.live_gate || q.tile_uni)
      throw std::runtime_error(std::string(pre) + "dense fused calls in place of one-class batches in the plain form, without poses");
    if (n_ticks != 0 && q.n_ticks != n_ticks) throw std::runtime_error(std::string(pre) + "every part runs the same number of ticks");
    n_ticks = q.n_ticks;
    if (gated ? (!q.fused_gate || !q.fused_gate_nis) : q.fused_gate != 0)
      throw std::runtime_error(std::string(pre) + "the gated loop needs every part's NIS rows, the plain loop has none");
    if ((dt_tab != nullptr) != (q.dt_sched != 0)) throw std::runtime_error(std::string(pre) + "one time-step table for every part, or none");
    if (dt_tab && (long)q.n_ticks > kDtTabMaxTicks) throw std::runtime_error(std::string(pre) + "more ticks than a table's offsets reach");
    waves_max = std::max(waves_max, (q.n + TPW - 1) / TPW);
  }
  static const long small_grid = [] { const char* e = std::getenv("TE_SMALL_GRID_WAVES"); return e ? std::atol(e) : 1024L; }();
  static const int nt_env = [] { const char* e = std::getenv("TE_NT_MEAS"); return e ? std::atoi(e) : -1; }();
  // (as for the single-batch launches: small, latency-bound grids spread one wavefront per workgroup over the CUs)
  const int wpb = waves_max <= small_grid ? 1 : 4;
  unsigned end = 0;
  for (int k = 0; k < 4; ++k) {
    StepParams q = parts[k];
    if (q.n <= 0) { q = StepParams{}; q.n = 0; }
    q.reverse = 0;   // (no fused call is reversed)
    p.part[k].a = make_step_args<T>(q);
    if (nt_env >= 0) p.part[k].a.nt_meas = nt_env;
    FusedGate& g = p.part[k].g;   // as OpsImpl::launch_fused_gate fills it; an empty part and the plain loop read none of it
    g.gate = q.fused_gate ? q.fused_gate_nis_max : 0.0;
    g.nis = q.fused_gate_nis; g.nis_stride = q.fused_gate_nis_stride; g.nis_ring = q.fused_gate_nis_ring;
    g.innov = q.fused_gate_innov; g.innov_ld = q.fused_gate_innov_ld; g.innov_stride = q.fused_gate_innov_stride;
    g.k = q.fused_gate ? q.fused_gate_k : -1; g.run = q.reacq_run; g.p0_tab = q.reacq_p0; g.p0_idx = q.reacq_p0_idx;
    // (a predict-only call changes no run and, like the single ticks, writes no event row)
    g.event = q.meas ? q.fused_gate_event : nullptr; g.event_stride = q.fused_gate_event_stride; g.event_ring = q.fused_gate_event_ring;
    p.part[k].dt_tab = dt_tab;
    const long waves = (q.n + TPW - 1) / TPW;
    end += (unsigned)((waves + wpb - 1) / wpb);
    p.end[k] = end;
  }
  if (end == 0) return;
  if (!population_fused_ok(sizeof(T) == 8, gated, dt_tab != nullptr)) throw std::runtime_error(std::string(pre) + "no kernel for this request");
  if (gated && dt_tab) launch_population_fused_grid<T, true, true>(p, end, (unsigned)wpb, s);
  else if (gated) launch_population_fused_grid<T, true, false>(p, end, (unsigned)wpb, s);
  else if (dt_tab) launch_population_fused_grid<T, false, true>(p, end, (unsigned)wpb, s);
  else launch_population_fused_grid<T, false, false>(p, end, (unsigned)wpb, s);
}

void launch_population_fused(int dtype, const StepParams parts[4], bool gated, const double* dt_tab, hipStream_t s) {
  if (dtype == F64) launch_population_fused_t<double>(parts, gated, dt_tab, s);
  else launch_population_fused_t<float>(parts, gated, dt_tab, s);
}

}  // namespace te
