// Host test of csrc/step_variant.hpp (no HIP): the launch plan of a FUSED request that carries a time-step schedule
// (StepParams::dt_sched), plain and with the fused gate, row by row, next to fused_gate_plan_host_test.cpp, whose request types
// have no such member and plan as they always did.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/dt_schedule_plan_host_test.cpp && ./a.out
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Old {   // (the request type of fused_gate_plan_host_test.cpp: no dt_sched)
  bool idx = false, cls = false, rec_out = false, q_delta = false, pose = false, nis = false;
  bool o_pose = false, o_twist = false, o_acc = false, done_flag = false, done_count = false;
  bool live_posted = false, live_mirror = false, live_progress = false, live_done = false, live_pose = false;
  bool tile_uni = false, tile_blk = false;
  long live_ring = 0;
  int n_ticks = 1;
  long n = 203;
  double gate = 0.0;
  int gate_by_writer = 0;
  int reacq = 0, reacq_k = 0;
  bool reacq_run = false, reacq_p0 = false, reacq_p0_idx = false, meas = true;
  int gate_id = 0, gate_id_k = -1;
  int live_gate = 0;
  double live_gate_nis_max = 0.0;
  bool live_gate_nis = false;
  long live_gate_nis_stride = 0, live_gate_nis_ring = 0;
  int live_gate_k = -1;
  bool live_gate_event = false;
  long live_gate_event_stride = 0, live_gate_event_ring = 0;
  int fused_gate = 0;
  double fused_gate_nis_max = 0.0;
  bool fused_gate_nis = false;
  long fused_gate_nis_stride = 0, fused_gate_nis_ring = 0;
  bool fused_gate_innov = false;
  long fused_gate_innov_ld = 0, fused_gate_innov_stride = 0;
  int fused_gate_k = -1;
  bool fused_gate_event = false;
  long fused_gate_event_stride = 0, fused_gate_event_ring = 0;
};
struct Req : Old {
  int dt_sched = 0;
  bool dt_host = false, dt_tab = false;
};

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++g_fail;                                            \
      std::printf("FAIL line %d: %s: ", __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
    }                                                      \
  } while (0)

// {sep, shared, uniform_tiles, has_live, fused_pose_tick_by_tick, fused_spills, tpw[, gate_by_writer[, fused_gate_tick_by_tick[,
//  fused_dt_tick_by_tick[, fused_gate_dt_tick_by_tick]]]]}
static const StepTraits kSepFull{true, false, false, false, false, false, 64};
static const StepTraits kSepPacked{true, false, false, true, false, false, 64};
static const StepTraits kSepPoseTicks{true, false, false, true, true, false, 64};
static const StepTraits kSepNoDt{true, false, false, true, false, false, 64, false, false, true, false};
static const StepTraits kSepNoGateDt{true, false, false, true, false, false, 64, false, false, false, true};
static const StepTraits kSepNoGate{true, false, false, true, false, false, 64, false, true};
static const StepTraits kSepWriter{true, false, false, true, false, false, 64, true};
static const StepTraits kSharedUt{true, true, true, false, false, false, 64};
static const StepTraits kDense{false, false, false, false, false, false, 64};
static const StepTraits kDenseSpills{false, false, false, false, false, true, 64};

template <class R>
static std::string run(const StepTraits& t, const R& r) {
  try {
    const StepPlan p = plan_step(t, r);
    std::string s = p.fused_gated ? "fused gate: " : p.live_gated ? "live gate: " : p.gate_by_id ? "by id: " : p.gated ? "gated: " : "";
    if (p.dt_table) s += "table, ";
    if (p.innov_writer_first) s += "innov, ";
    if (p.reacquire_after_step) s += "reacquire, ";
    if (p.tick_by_tick) s += std::to_string(r.n_ticks) + " x ";
    return s + "(" + std::to_string(p.variant) + (p.pose_writer_after_each_tick ? " + pose)" : ")");
  } catch (const std::runtime_error&) {
    return "throws";
  }
}
#define PIN(traits, req, want) CHECK(run(traits, req) == (want), "%s, want %s", run(traits, req).c_str(), std::string(want).c_str())

int main() {
  static_assert(has_dt_sched_member<Req>::value && !has_dt_sched_member<Old>::value, "the member-detection helper");
  static_assert(!StepPlan{}.dt_table, "the new field defaults to false");
  static_assert(!StepTraits{true, false, false, true, false, false, 64}.fused_dt_tick_by_tick &&
                    !StepTraits{true, false, false, true, false, false, 64}.fused_gate_dt_tick_by_tick, "the new traits default to false");
  static_assert(kVariantBits == 9, "the schedule is a template argument next to the variant word: no new bit");
  const std::string F = std::to_string((unsigned)kFused);
  const std::string one = "table, (" + F + ")", ticks = "20 x (0)";
  const std::string gone = "fused gate: table, (" + F + ")", gticks = "fused gate: 20 x (0)";
  Req d;
  d.n_ticks = 20;
  d.dt_sched = 1; d.dt_host = d.dt_tab = true;
  Req g = d;
  g.fused_gate = 1; g.fused_gate_nis_max = 300.0; g.fused_gate_nis = true; g.fused_gate_nis_stride = 256;
  g.fused_gate_k = 3; g.reacq_run = g.reacq_p0 = g.reacq_p0_idx = true;
  // ---- one launch where the traits allow it: the plain loop and the gated loop, both separable layouts, one tick included,
  // masked or predict only; a trait that concerns the other loop, the pose kernels or the scalar fused gate only does not matter
  for (const StepTraits* t : {&kSepFull, &kSepPacked}) {
    PIN(*t, d, one);
    PIN(*t, g, gone);
    { Req r = d; r.n_ticks = 1; PIN(*t, r, one); }          // (a single tick with a table is the kFused loop of one tick)
    { Req r = g; r.n_ticks = 1; PIN(*t, r, gone); }
    { Req r = d; r.meas = false; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_k = -1; r.fused_gate_nis_max = 0.0; PIN(*t, r, gone); }   // the plain innovation stream
  }
  PIN(kSepPoseTicks, d, one);
  PIN(kSepNoGateDt, d, one);
  PIN(kSepNoGate, d, one);
  PIN(kSepNoDt, g, gone);
  {   // the plans' flags
    const StepPlan p = plan_step(kSepPacked, d);
    CHECK(p.dt_table && p.variant == kFused && !p.tick_by_tick && !p.fused_gated && !p.gated && !p.innov_writer_first && !p.pose_writer_after_each_tick, "flags");
    const StepPlan q = plan_step(kSepPacked, g);
    CHECK(q.dt_table && q.variant == kFused && !q.tick_by_tick && q.fused_gated && !q.gated, "flags of the gated plan");
  }
  // ---- tick by tick inside the call: a call with poses; the dense layouts and the symmetric-packed EKF (the dense kernels);
  // several (Q, R) classes; a flagged instantiation
  { Req r = d; r.pose = true; PIN(kSepPacked, r, "20 x (" + std::to_string((unsigned)kPose) + ")"); PIN(kSepFull, r, "20 x (" + std::to_string((unsigned)kPose) + ")");
    PIN(kDense, r, "20 x (0 + pose)"); }
  { Req r = g; r.pose = true; PIN(kSepPacked, r, gticks); PIN(kSepFull, r, gticks); }
  for (const StepTraits* t : {&kDense, &kDenseSpills}) { PIN(*t, d, ticks); PIN(*t, g, gticks); }
  { Req r = d; r.cls = true; PIN(kSepPacked, r, "20 x (" + std::to_string((unsigned)kPerQR) + ")"); PIN(kDense, r, "20 x (" + std::to_string((unsigned)kPerQR) + ")"); }
  { Req r = g; r.cls = true; PIN(kSepPacked, r, gticks); PIN(kDense, r, gticks); }
  PIN(kSepNoDt, d, ticks);
  PIN(kSepNoGateDt, g, gticks);
  PIN(kSepNoGate, g, gticks);     // (no scalar fused gated kernel: none with a table either)
  PIN(kSepWriter, g, gticks);
  {
    const StepPlan p = plan_step(kDense, d);
    CHECK(!p.dt_table && p.tick_by_tick && p.variant == 0 && !p.fused_gated, "flags of the tick-by-tick plan");
    { Req r = d; r.n_ticks = 1; const StepPlan q = plan_step(kDense, r); CHECK(!q.dt_table && q.tick_by_tick && q.variant == 0, "one tick, dense"); }
  }
  // a tick-by-tick plan needs no device table; a one-launch plan does; both need the host's array
  { Req r = d; r.dt_tab = false; PIN(kDense, r, ticks); PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.dt_tab = false; PIN(kDense, r, gticks); PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.dt_host = false; PIN(kDense, r, "throws"); PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.dt_host = false; PIN(kDense, r, "throws"); PIN(kSepPacked, r, "throws"); }
  // ---- refused: what a dense fused launch in place is not
  PIN(kSharedUt, d, "throws");   // (the batch is expanded first)
  PIN(kSharedUt, g, "throws");
  { Req r = d; r.idx = true; PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.rec_out = true; PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.q_delta = true; PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.nis = true; PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.nis = true; r.gate = 300.0; PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.n_ticks = 0; PIN(kSepPacked, r, "throws"); }
  { Req r = d; r.live_posted = r.live_mirror = r.live_progress = r.live_done = true; r.live_ring = 8; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_k = 128; PIN(kSepPacked, r, "throws"); }   // (the fused gate's own refusals hold with a schedule)
  { Req r = g; r.fused_gate_nis = false; PIN(kSepPacked, r, "throws"); }
  // ---- dt_sched 0: the other members are not read, the request plans as it always did
  { Req r; r.n_ticks = 20; r.dt_tab = true; PIN(kSepPacked, r, "(" + F + ")"); PIN(kDenseSpills, r, ticks); PIN(kDense, r, "(" + F + ")"); }
  { Req r = g; r.dt_sched = 0; PIN(kSepPacked, r, "fused gate: (" + F + ")"); PIN(kDense, r, gticks); }
  { Req r; PIN(kSepPacked, r, "(0)"); }
  // ---- a request type WITHOUT the member plans as it always did
  { Old o; o.n_ticks = 20; PIN(kSepPacked, o, "(" + F + ")"); PIN(kDense, o, "(" + F + ")"); PIN(kDenseSpills, o, ticks); PIN(kSharedUt, o, "throws"); }
  { Old o; o.n_ticks = 20; o.pose = true; PIN(kSepPacked, o, "(" + std::to_string((unsigned)(kFused | kPose)) + ")"); PIN(kSepPoseTicks, o, "20 x (" + std::to_string((unsigned)kPose) + ")"); }
  { Old o = g; PIN(kSepPacked, o, "fused gate: (" + F + ")"); PIN(kDense, o, gticks); }
  { Old o; o.nis = true; o.gate = 300.0; PIN(kSepPacked, o, "gated: (" + std::to_string((unsigned)kInnov) + ")"); }
  { Old o; PIN(kSepPacked, o, "(0)"); PIN(kDense, o, "(0)"); }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("dt schedule plan host test ok\n");
  return 0;
}
