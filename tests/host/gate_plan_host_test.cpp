// Host test of csrc/step_variant.hpp (no HIP): the launch plan of a request with a validation gate (StepParams::gate), row by
// row, next to tests/host/step_variant_host_test.cpp, whose request type has no gate member and plans as it always did.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/gate_plan_host_test.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Old {   // (the request type of step_variant_host_test.cpp: no gate)
  bool idx = false, cls = false, rec_out = false, q_delta = false, pose = false, nis = false;
  bool o_pose = false, o_twist = false, o_acc = false, done_flag = false, done_count = false;
  bool live_posted = false, live_mirror = false, live_progress = false, live_done = false, live_pose = false;
  bool tile_uni = false, tile_blk = false;
  long live_ring = 0;
  int n_ticks = 1;
  long n = 65;
};
struct Req : Old {
  double gate = 0.0;
  int gate_by_writer = 0;
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
static const StepTraits kSepRouted{true, false, false, true, false, false, 64, true};   // a gated kernel that would spill: by the writer
static const StepTraits kDense{false, false, false, false, false, false, 64};
static const StepTraits kDenseG6{false, false, false, false, false, false, 10};

// "gated: innov, (8 + pose)" -- the variant in decimal
template <class R>
static std::string run(const StepTraits& t, const R& r) {
  try {
    const StepPlan p = plan_step(t, r);
    std::string s = p.gated ? "gated: " : "";
    if (p.innov_writer_first) s += "innov, ";
    if (p.tick_by_tick) s += std::to_string(r.n_ticks) + " x ";
    return s + "(" + std::to_string(p.variant) + (p.pose_writer_after_each_tick ? " + pose)" : ")");
  } catch (const std::runtime_error&) {
    return "throws";
  }
}
#define PIN(traits, req, want) CHECK(run(traits, req) == (want), "%s, want %s", run(traits, req).c_str(), std::string(want).c_str())

int main() {
  const std::string innov = std::to_string((unsigned)kInnov), perqr = std::to_string((unsigned)kPerQR);
  static_assert(has_gate_member<Req>::value && !has_gate_member<Old>::value, "the member-detection helper");
  Req g;
  g.nis = true; g.gate = 11.345;
  // separable, one class: the gated kInnov kernel, no writer
  for (const StepTraits* t : {&kSepFull, &kSepPacked, &kSharedUt}) PIN(*t, g, "gated: (" + innov + ")");
  { Req r = g; r.tile_uni = r.tile_blk = true; PIN(kSharedUt, r, "gated: (" + innov + ")"); }
  { Req r = g; r.gate = std::numeric_limits<double>::infinity(); PIN(kSepPacked, r, "gated: (" + innov + ")"); }
  // + pose: the pose writer behind the step
  { Req r = g; r.pose = true; PIN(kSepPacked, r, "gated: (" + innov + " + pose)"); }
  // several classes, the dense kernels, a routed instantiation, a caller that asks for the row: writer first, plain step
  { Req r = g; r.cls = true; PIN(kSepPacked, r, "gated: innov, (" + perqr + ")"); }
  { Req r = g; r.cls = true; r.pose = true; PIN(kSepPacked, r, "gated: innov, (" + perqr + " + pose)"); }
  PIN(kDense, g, "gated: innov, (0)");
  PIN(kDenseG6, g, "gated: innov, (0)");
  { Req r = g; r.cls = true; PIN(kDense, r, "gated: innov, (" + perqr + ")"); }
  PIN(kSepRouted, g, "gated: innov, (0)");
  { Req r = g; r.gate_by_writer = 1; PIN(kSepPacked, r, "gated: innov, (0)"); }
  // gate 0: the innovation stream's plan
  { Req r = g; r.gate = 0.0; PIN(kSepPacked, r, "(" + innov + ")"); PIN(kDense, r, "innov, (0)"); PIN(kSepRouted, r, "(" + innov + ")"); }
  // refused: a gate without the NIS row; negative, NaN; with idx, several ticks, a live launch, the getter table, A -> B, the fused query
  for (const StepTraits* t : {&kSepPacked, &kDense}) {
    { Req r = g; r.nis = false; PIN(*t, r, "throws"); }
    { Req r = g; r.gate = -1.0; PIN(*t, r, "throws"); }
    { Req r = g; r.gate = std::nan(""); PIN(*t, r, "throws"); }
    { Req r; r.gate = -1.0; PIN(*t, r, "throws"); }
    { Req r = g; r.idx = true; PIN(*t, r, "throws"); }
    { Req r = g; r.n_ticks = 3; PIN(*t, r, "throws"); }
    { Req r = g; r.live_posted = r.live_mirror = r.live_progress = r.live_done = true; r.live_ring = 8; r.n_ticks = 3; PIN(*t, r, "throws"); }
    { Req r = g; r.idx = r.o_pose = r.o_twist = r.o_acc = r.done_flag = r.done_count = true; PIN(*t, r, "throws"); }
    { Req r = g; r.rec_out = true; PIN(*t, r, "throws"); }
    { Req r = g; r.q_delta = true; PIN(*t, r, "throws"); }
  }
  // a request type without the member plans as before, whatever the traits say about the gate
  {
    Old o;
    PIN(kSepPacked, o, "(0)");
    PIN(kSepRouted, o, "(0)");
    o.nis = true;
    PIN(kSepPacked, o, "(" + innov + ")");
    PIN(kSepRouted, o, "(" + innov + ")");
    PIN(kDense, o, "innov, (0)");
    o.pose = true;
    PIN(kSepPacked, o, "(" + innov + " + pose)");
  }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("gate plan host test ok\n");
  return 0;
}
