// Host test of csrc/step_variant.hpp (no HIP): the launch plan of a RESIDENT request that carries the gate of its session
// (StepParams::live_gate), row by row, next to gate_plan_host_test.cpp and update_gate_plan_host_test.cpp, whose request types
// have no such member and plan as they always did.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/live_gate_plan_host_test.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Old {   // (the request type of update_gate_plan_host_test.cpp: gates and policies of the launched calls, no live_gate)
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
};
struct Req : Old {
  int live_gate = 0;
  double live_gate_nis_max = 0.0;
  bool live_gate_nis = false;
  long live_gate_nis_stride = 0, live_gate_nis_ring = 0;
  int live_gate_k = -1;
  bool live_gate_event = false;
  long live_gate_event_stride = 0, live_gate_event_ring = 0;
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

// {sep, shared, uniform_tiles, has_live, fused_pose_tick_by_tick, fused_spills, tpw[, gate_by_writer]}
static const StepTraits kSepFull{true, false, false, false, false, false, 64};
static const StepTraits kSepPacked{true, false, false, true, false, false, 64};
static const StepTraits kSharedUt{true, true, true, false, false, false, 64};
static const StepTraits kDense{false, false, false, false, false, false, 64};

template <class R>
static std::string run(const StepTraits& t, const R& r) {
  try {
    const StepPlan p = plan_step(t, r);
    std::string s = p.live_gated ? "live gate: " : p.gate_by_id ? "by id: " : p.gated ? "gated: " : "";
    if (p.innov_writer_first) s += "innov, ";
    if (p.reacquire_after_step) s += "reacquire, ";
    if (p.tick_by_tick) s += std::to_string(r.n_ticks) + " x ";
    return s + "(" + std::to_string(p.variant) + (p.pose_writer_after_each_tick ? " + pose)" : ")");
  } catch (const std::runtime_error&) {
    return "throws";
  }
}
#define PIN(traits, req, want) CHECK(run(traits, req) == (want), "%s, want %s", run(traits, req).c_str(), std::string(want).c_str())

template <class R>
static R live() {   // a resident request over a ring of 8
  R r;
  r.live_posted = r.live_mirror = r.live_progress = r.live_done = true;
  r.live_ring = 8; r.n_ticks = 20;
  return r;
}

int main() {
  static_assert(has_live_gate_member<Req>::value && !has_live_gate_member<Old>::value, "the member-detection helper");
  static_assert(!StepPlan{}.live_gated, "the new field defaults to false");
  static_assert(sep_variant_ok(kFused | kLive2, false) && !sep_variant_ok(kFused | kLive2 | kInnov, false) && !sep_variant_ok(kFused | kLive1 | kInnov, false),
                "the variant word stays kFused | kLive2: kInnov never meets kLive");
  const std::string l1 = "(" + std::to_string((unsigned)(kFused | kLive1)) + ")", l2 = "(" + std::to_string((unsigned)(kFused | kLive2)) + ")";
  const std::string gated = "live gate: " + l2;
  Req g = live<Req>();
  g.live_gate = 1; g.live_gate_nis_max = 300.0; g.live_gate_nis = true;
  // ---- accepted: gate only, count only, K, with event rows, with the pose output / query of the same session, +inf
  PIN(kSepPacked, g, gated);
  { Req r = g; r.live_gate_k = 0; r.reacq_run = true; PIN(kSepPacked, r, gated); }
  { Req r = g; r.live_gate_k = 3; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(kSepPacked, r, gated); }
  { Req r = g; r.live_gate_k = 127; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; r.live_gate_event = true; r.live_gate_event_stride = 256; r.live_gate_event_ring = 8; PIN(kSepPacked, r, gated); }
  { Req r = g; r.live_pose = true; PIN(kSepPacked, r, gated); }
  { Req r = g; r.q_delta = true; PIN(kSepPacked, r, gated); }
  { Req r = g; r.live_gate_nis_max = std::numeric_limits<double>::infinity(); PIN(kSepPacked, r, gated); }
  { Req r = g; r.live_gate_nis_stride = 256; r.live_gate_nis_ring = 8; PIN(kSepPacked, r, gated); }
  {   // the plan's flags
    const StepPlan p = plan_step(kSepPacked, g);
    CHECK(p.live_gated && p.variant == (kFused | kLive2) && !p.gated && !p.gate_by_id && !p.innov_writer_first && !p.reacquire_after_step && !p.tick_by_tick &&
              !p.pose_writer_after_each_tick, "flags");
  }
  // ---- refused
  { Req r = g; r.idx = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.cls = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.rec_out = true; PIN(kSepPacked, r, "throws"); }
  for (const StepTraits* t : {&kSepFull, &kSharedUt, &kDense}) PIN(*t, g, "throws");   // kinds without live kernels
  { Req r = g; r.live_posted = false; PIN(kSepPacked, r, "throws"); }                  // the resident gate outside a resident launch
  { Req r = g; r.live_gate_nis_max = 0.0; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_nis_max = -1.0; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_nis_max = std::nan(""); PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_nis = false; PIN(kSepPacked, r, "throws"); }                // no NIS rows
  { Req r = g; r.live_gate_nis_stride = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_nis_ring = -1; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_k = -2; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_k = 128; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_gate_k = 0; PIN(kSepPacked, r, "throws"); }                      // runs without the run row
  { Req r = g; r.live_gate_k = 3; r.reacq_run = true; PIN(kSepPacked, r, "throws"); }  // re-initialisation without the P0 table
  { Req r = g; r.live_gate_event = true; PIN(kSepPacked, r, "throws"); }               // event rows without a policy
  { Req r = g; r.nis = true; PIN(kSepPacked, r, "throws"); }                           // the launched calls' stream: kInnov never meets kLive
  { Req r = g; r.gate = 300.0; r.nis = true; PIN(kSepPacked, r, "throws"); }           // ... nor their gate (gate_plan_host_test.cpp:92)
  { Req r = g; r.gate = 300.0; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.reacq = 1; r.reacq_k = 3; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(kSepPacked, r, "throws"); }
  { Req r = g; r.live_ring = 0; PIN(kSepPacked, r, "throws"); }                        // what a plain resident launch is refused for
  { Req r = g; r.live_mirror = false; PIN(kSepPacked, r, "throws"); }
  // ---- live_gate 0: the other members are not read, the request plans as a plain resident one
  { Req r = live<Req>(); r.live_gate_k = 3; r.live_gate_nis_max = 300.0; PIN(kSepPacked, r, l1); }
  { Req r = live<Req>(); r.live_pose = true; PIN(kSepPacked, r, l2); }
  // ---- a request type WITHOUT the member plans as it always did
  { Old o = live<Old>(); PIN(kSepPacked, o, l1); PIN(kSepFull, o, "throws"); PIN(kDense, o, "throws"); }
  { Old o = live<Old>(); o.live_pose = true; PIN(kSepPacked, o, l2); }
  { Old o = live<Old>(); o.q_delta = true; PIN(kSepPacked, o, l2); }
  { Old o = live<Old>(); o.gate = 300.0; o.nis = true; PIN(kSepPacked, o, "throws"); }
  { Old o; o.nis = true; o.gate = 300.0; PIN(kSepPacked, o, "gated: (" + std::to_string((unsigned)kInnov) + ")"); PIN(kDense, o, "gated: innov, (0)"); }
  { Old o; o.idx = o.nis = true; o.gate = 300.0; o.gate_id = 1; PIN(kSepPacked, o, "by id: (" + std::to_string((unsigned)(kInnov | kIndexed)) + ")"); }
  { Old o; PIN(kSepPacked, o, "(0)"); PIN(kDense, o, "(0)"); }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("live gate plan host test ok\n");
  return 0;
}
