// Host test of csrc/step_variant.hpp (no HIP): the launch plan of a FUSED request that carries the gate, the innovation stream and
// the policy of its call (StepParams::fused_gate), row by row, next to live_gate_plan_host_test.cpp, whose request types have no
// such member and plan as they always did.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/fused_gate_plan_host_test.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Old {   // (the request type of live_gate_plan_host_test.cpp: no fused_gate)
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
};
struct Req : Old {
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

// {sep, shared, uniform_tiles, has_live, fused_pose_tick_by_tick, fused_spills, tpw[, gate_by_writer[, fused_gate_tick_by_tick]]}
static const StepTraits kSepFull{true, false, false, false, false, false, 64};
static const StepTraits kSepPacked{true, false, false, true, false, false, 64};
static const StepTraits kSepFlagged{true, false, false, true, false, false, 64, false, true};
static const StepTraits kSepWriter{true, false, false, true, false, false, 64, true};
static const StepTraits kSharedUt{true, true, true, false, false, false, 64};
static const StepTraits kDense{false, false, false, false, false, false, 64};
static const StepTraits kDenseSpills{false, false, false, false, false, true, 64};

template <class R>
static std::string run(const StepTraits& t, const R& r) {
  try {
    const StepPlan p = plan_step(t, r);
    std::string s = p.fused_gated ? "fused gate: " : p.live_gated ? "live gate: " : p.gate_by_id ? "by id: " : p.gated ? "gated: " : "";
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
  static_assert(has_fused_gate_member<Req>::value && !has_fused_gate_member<Old>::value, "the member-detection helper");
  static_assert(!StepPlan{}.fused_gated, "the new field defaults to false");
  static_assert(!StepTraits{true, false, false, true, false, false, 64}.fused_gate_tick_by_tick, "the new trait defaults to false");
  static_assert(sep_variant_ok(kFused, false) && !sep_variant_ok(kFused | kInnov, false) && !sep_variant_ok(kFused | kInnov | kPose, false),
                "the variant word stays kFused (the gate is a template argument next to it): kInnov never meets kFused");
  static_assert(!variant_in(kSepVariants, kFused | kInnov), "... and the variant list ships no such kernel");
  const std::string one = "fused gate: (" + std::to_string((unsigned)kFused) + ")", ticks = "fused gate: 20 x (0)";
  Req g;
  g.n_ticks = 20;
  g.fused_gate = 1; g.fused_gate_nis_max = 300.0; g.fused_gate_nis = true; g.fused_gate_nis_stride = 256;
  // ---- accepted, one launch: gate only, with innovation blocks, count only, K, with event rows, rings, +inf, no gate, one tick, predict only
  for (const StepTraits* t : {&kSepFull, &kSepPacked}) {
    PIN(*t, g, one);
    { Req r = g; r.fused_gate_innov = true; r.fused_gate_innov_ld = 256; r.fused_gate_innov_stride = 6 * 256; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_k = 0; r.reacq_run = true; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_k = 3; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_k = 127; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; r.fused_gate_event = true; r.fused_gate_event_stride = 256; r.fused_gate_event_ring = 8; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_nis_ring = 8; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_nis_stride = 0; PIN(*t, r, one); }
    { Req r = g; r.fused_gate_nis_max = std::numeric_limits<double>::infinity(); PIN(*t, r, one); }
    { Req r = g; r.fused_gate_nis_max = 0.0; PIN(*t, r, one); }   // the plain innovation stream from a fused call
    { Req r = g; r.n_ticks = 1; PIN(*t, r, one); }
    { Req r = g; r.meas = false; PIN(*t, r, one); }
  }
  {   // the plan's flags
    const StepPlan p = plan_step(kSepPacked, g);
    CHECK(p.fused_gated && p.variant == kFused && !p.gated && !p.live_gated && !p.gate_by_id && !p.innov_writer_first && !p.reacquire_after_step &&
              !p.tick_by_tick && !p.pose_writer_after_each_tick, "flags");
  }
  // ---- accepted, tick by tick inside the call: the dense layouts, several (Q, R) classes, a flagged instantiation, a layout whose
  // gate is the writer's, a pose stream in the same call
  for (const StepTraits* t : {&kDense, &kDenseSpills, &kSepFlagged, &kSepWriter}) PIN(*t, g, ticks);
  { Req r = g; r.cls = true; PIN(kSepPacked, r, ticks); PIN(kDense, r, ticks); }
  { Req r = g; r.pose = true; PIN(kSepPacked, r, ticks); PIN(kSepFull, r, ticks); }
  {
    const StepPlan p = plan_step(kDense, g);
    CHECK(p.fused_gated && p.tick_by_tick && p.variant == 0 && !p.gated && !p.innov_writer_first, "flags of the tick-by-tick plan");
  }
  // ---- refused
  PIN(kSharedUt, g, "throws");   // (the batch is expanded first)
  { Req r = g; r.idx = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.rec_out = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.q_delta = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.o_pose = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.tile_uni = r.tile_blk = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.n_ticks = 0; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_posted = r.live_mirror = r.live_progress = r.live_done = true; r.live_ring = 8; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_nis_max = -1.0; PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }
  { Req r = g; r.fused_gate_nis_max = std::nan(""); PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }
  { Req r = g; r.fused_gate_nis = false; PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }   // a gate without the NIS row
  { Req r = g; r.fused_gate_nis_stride = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_nis_ring = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_innov = true; r.fused_gate_innov_ld = 202; PIN(kSepPacked, r, "throws"); }   // ld < n
  { Req r = g; r.fused_gate_innov = true; r.fused_gate_innov_ld = 256; r.fused_gate_innov_stride = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_k = -2; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_k = 128; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }
  { Req r = g; r.fused_gate_k = 0; r.reacq_run = true; r.fused_gate_nis_max = 0.0; PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }   // a policy without a gate
  { Req r = g; r.fused_gate_k = 0; PIN(kSepPacked, r, "throws"); }                      // runs without the run row
  { Req r = g; r.fused_gate_k = 3; r.reacq_run = true; PIN(kSepPacked, r, "throws"); }  // re-initialisation without the P0 table
  { Req r = g; r.fused_gate_event = true; PIN(kSepPacked, r, "throws"); }               // event rows without a policy
  { Req r = g; r.fused_gate_k = 0; r.reacq_run = true; r.fused_gate_event = true; r.fused_gate_event_stride = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.fused_gate_k = 0; r.reacq_run = true; r.fused_gate_event = true; r.fused_gate_event_ring = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.nis = true; PIN(kSepPacked, r, "throws"); }                            // the single ticks' stream ...
  { Req r = g; r.gate = 300.0; r.nis = true; PIN(kSepPacked, r, "throws"); }            // ... their gate ...
  { Req r = g; r.gate = 300.0; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.reacq = 1; r.reacq_k = 3; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(kSepPacked, r, "throws"); }   // ... their policy
  { Req r = g; r.gate_by_writer = 1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate = 1; r.live_gate_nis_max = 300.0; r.live_gate_nis = true; PIN(kSepPacked, r, "throws"); }
  // ---- fused_gate 0: the other members are not read, the request plans as it always did; gate > 0 or nis with n_ticks > 1 stays refused
  const std::string fused = "(" + std::to_string((unsigned)kFused) + ")", innov = std::to_string((unsigned)kInnov);
  { Req r; r.n_ticks = 20; r.fused_gate_k = 3; r.fused_gate_nis_max = 300.0; PIN(kSepPacked, r, fused); PIN(kDenseSpills, r, "20 x (0)"); }
  { Req r; r.n_ticks = 20; r.gate = 300.0; r.nis = true; PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }
  { Req r; r.n_ticks = 20; r.nis = true; PIN(kSepPacked, r, "throws"); PIN(kDense, r, "throws"); }
  { Req r; r.nis = true; r.gate = 300.0; PIN(kSepPacked, r, "gated: (" + innov + ")"); PIN(kDense, r, "gated: innov, (0)"); }
  // ---- a request type WITHOUT the member plans as it always did
  { Old o; o.n_ticks = 20; PIN(kSepPacked, o, fused); PIN(kDense, o, fused); PIN(kDenseSpills, o, "20 x (0)"); PIN(kSharedUt, o, "throws"); }
  { Old o; o.n_ticks = 20; o.pose = true; PIN(kSepPacked, o, "(" + std::to_string((unsigned)(kFused | kPose)) + ")"); PIN(kDense, o, "20 x (0 + pose)"); }
  { Old o; o.n_ticks = 20; o.gate = 300.0; o.nis = true; PIN(kSepPacked, o, "throws"); PIN(kSepFull, o, "throws"); PIN(kDense, o, "throws"); }
  { Old o; o.n_ticks = 20; o.nis = true; PIN(kSepPacked, o, "throws"); PIN(kDense, o, "throws"); }
  { Old o; o.n_ticks = 20; o.gate = 300.0; PIN(kSepPacked, o, "throws"); }
  { Old o; o.nis = true; o.gate = 300.0; PIN(kSepPacked, o, "gated: (" + innov + ")"); PIN(kDense, o, "gated: innov, (0)"); }
  { Old o; o.nis = true; o.gate = 300.0; o.reacq = 1; o.reacq_k = 3; o.reacq_run = o.reacq_p0 = o.reacq_p0_idx = true; PIN(kSepPacked, o, "gated: reacquire, (" + innov + ")"); }
  { Old o; o.idx = o.nis = true; o.gate = 300.0; o.gate_id = 1; PIN(kSepPacked, o, "by id: (" + std::to_string((unsigned)(kInnov | kIndexed)) + ")"); }
  { Old o; PIN(kSepPacked, o, "(0)"); PIN(kDense, o, "(0)"); }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("fused gate plan host test ok\n");
  return 0;
}
