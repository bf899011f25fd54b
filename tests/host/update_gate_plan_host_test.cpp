// Host test of csrc/step_variant.hpp (no HIP): the launch plan of an INDEXED request that carries the by-id update policy
// (StepParams::gate_id), row by row, next to gate_plan_host_test.cpp and reacquire_plan_host_test.cpp, whose request types have
// no such member and plan as they always did.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/update_gate_plan_host_test.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Gated {   // (the request type of gate_plan_host_test.cpp: a gate, no policy by id)
  bool idx = false, cls = false, rec_out = false, q_delta = false, pose = false, nis = false;
  bool o_pose = false, o_twist = false, o_acc = false, done_flag = false, done_count = false;
  bool live_posted = false, live_mirror = false, live_progress = false, live_done = false, live_pose = false;
  bool tile_uni = false, tile_blk = false;
  long live_ring = 0;
  int n_ticks = 1;
  long n = 65;
  double gate = 0.0;
  int gate_by_writer = 0;
};
struct Req : Gated {
  int reacq = 0, reacq_k = 0;
  bool reacq_run = false, reacq_p0 = false, reacq_p0_idx = false, meas = true;
  int gate_id = 0, gate_id_k = -1;
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
static const StepTraits kSepRouted{true, false, false, true, false, false, 64, true};
static const StepTraits kDense{false, false, false, false, false, false, 64};
static const StepTraits kDenseG6{false, false, false, false, false, false, 10};

template <class R>
static std::string run(const StepTraits& t, const R& r) {
  try {
    const StepPlan p = plan_step(t, r);
    std::string s = p.gate_by_id ? "by id: " : p.gated ? "gated: " : "";
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
  static_assert(has_gate_id_member<Req>::value && !has_gate_id_member<Gated>::value, "the member-detection helper");
  static_assert(sep_variant_ok(kInnov | kIndexed, false) && sep_variant_ok(kInnov | kIndexed, true), "the gated by-id step is a legal variant");
  static_assert(!variant_in(kSepVariants, kInnov | kIndexed), "... that the variant list does not ship as a plain kernel");
  static_assert(!sep_variant_ok(kInnov | kIndexed | kFused, false) && !sep_variant_ok(kInnov | kIndexed | kPerQR, false) &&
                    !sep_variant_ok(kInnov | kIndexed | kPose, false) && !sep_variant_ok(kInnov | kIndexed | kQuery, false) &&
                    !sep_variant_ok(kInnov | kIndexed | kAB, false) && !dense_variant_ok(kInnov | kIndexed),
                "and nothing else rides on it");
  const std::string byid = "by id: (" + std::to_string((unsigned)(kInnov | kIndexed)) + ")";
  const std::string innov = std::to_string((unsigned)kInnov);
  Req g;
  g.idx = g.nis = true; g.gate = 300.0; g.gate_id = 1;
  // ---- accepted: gate only, count only, K; every separable form; with the fused getter table; +inf
  for (const StepTraits* t : {&kSepFull, &kSepPacked, &kSharedUt}) {
    PIN(*t, g, byid);
    { Req r = g; r.gate_id_k = 0; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(*t, r, byid); }
    { Req r = g; r.gate_id_k = 127; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(*t, r, byid); }
    { Req r = g; r.o_pose = r.o_twist = r.o_acc = r.done_flag = r.done_count = true; PIN(*t, r, byid); }
    { Req r = g; r.o_pose = r.o_twist = r.o_acc = r.done_flag = true; r.n = 64; PIN(*t, r, byid); }
    { Req r = g; r.gate = std::numeric_limits<double>::infinity(); PIN(*t, r, byid); }
  }
  {   // the plan's flags
    const StepPlan p = plan_step(kSepPacked, g);
    CHECK(p.gate_by_id && p.gated && !p.innov_writer_first && !p.reacquire_after_step && !p.tick_by_tick && !p.pose_writer_after_each_tick, "flags");
  }
  // ---- refused under the policy
  for (const StepTraits* t : {&kSepPacked, &kSharedUt}) {
    { Req r = g; r.gate = 0.0; PIN(*t, r, "throws"); }                       // a policy without the gate
    { Req r = g; r.gate = -1.0; PIN(*t, r, "throws"); }
    { Req r = g; r.gate = std::nan(""); PIN(*t, r, "throws"); }
    { Req r = g; r.nis = false; PIN(*t, r, "throws"); }                      // no NIS row
    { Req r = g; r.idx = false; PIN(*t, r, "throws"); }                      // the policy is for indexed launches
    { Req r = g; r.gate_id_k = -2; PIN(*t, r, "throws"); }
    { Req r = g; r.gate_id_k = 128; PIN(*t, r, "throws"); }
    { Req r = g; r.gate_id_k = 3; PIN(*t, r, "throws"); }                    // runs without the run row and the P0 table
    { Req r = g; r.gate_id_k = 3; r.reacq_run = r.reacq_p0 = true; PIN(*t, r, "throws"); }
    { Req r = g; r.cls = true; PIN(*t, r, "throws"); }                       // several (Q, R) classes
    { Req r = g; r.n_ticks = 3; PIN(*t, r, "throws"); }
    { Req r = g; r.rec_out = true; PIN(*t, r, "throws"); }
    { Req r = g; r.q_delta = true; PIN(*t, r, "throws"); }
    { Req r = g; r.pose = true; PIN(*t, r, "throws"); }
    { Req r = g; r.tile_uni = r.tile_blk = true; PIN(*t, r, "throws"); }
    { Req r = g; r.gate_by_writer = 1; PIN(*t, r, "throws"); }               // (a batch that keeps measured-pose rows)
    { Req r = g; r.reacq = 1; r.reacq_k = 3; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true; PIN(*t, r, "throws"); }   // not both policies
    { Req r = g; r.live_posted = r.live_mirror = r.live_progress = r.live_done = true; r.live_ring = 8; PIN(*t, r, "throws"); }
    { Req r = g; r.o_pose = r.o_twist = r.o_acc = r.done_flag = true; r.n = 65; PIN(*t, r, "throws"); }   // the getter table's own rule
    { Req r = g; r.o_pose = true; PIN(*t, r, "throws"); }
  }
  PIN(kDense, g, "throws");        // the dense kf_step_kernel layouts, the symmetric-packed EKF among them
  PIN(kDenseG6, g, "throws");
  PIN(kSepRouted, g, "throws");    // an instantiation whose gate is the writer's mask row
  // ---- everything refused before stays refused for a request WITHOUT the policy, whatever type it has
  for (const StepTraits* t : {&kSepPacked, &kSharedUt, &kDense}) {
    Req r;
    r.nis = true; r.gate = 300.0;
    { Req q = r; q.idx = true; PIN(*t, q, "throws"); }                                                   // a gate on an indexed request
    { Req q = r; q.idx = q.o_pose = q.o_twist = q.o_acc = q.done_flag = q.done_count = true; PIN(*t, q, "throws"); }
    { Req q = r; q.gate = 0.0; q.idx = true; PIN(*t, q, "throws"); }                                     // an innovation stream on one
    { Req q = r; q.n_ticks = 3; PIN(*t, q, "throws"); }
    { Req q = r; q.rec_out = true; PIN(*t, q, "throws"); }
    { Req q = r; q.q_delta = true; PIN(*t, q, "throws"); }
    Gated o;
    o.nis = true; o.gate = 300.0; o.idx = true;
    PIN(*t, o, "throws");
    o.gate = 0.0;
    PIN(*t, o, "throws");
  }
  // ... and what was planned before is planned as before
  { Req r; r.nis = true; r.gate = 300.0; PIN(kSepPacked, r, "gated: (" + innov + ")"); PIN(kDense, r, "gated: innov, (0)"); }
  { Req r; r.nis = true; r.gate = 300.0; r.reacq = 1; r.reacq_k = 3; r.reacq_run = r.reacq_p0 = r.reacq_p0_idx = true;
    PIN(kSepPacked, r, "gated: reacquire, (" + innov + ")"); }
  { Req r; r.idx = true; PIN(kSepPacked, r, "(" + std::to_string((unsigned)kIndexed) + ")"); PIN(kDense, r, "(" + std::to_string((unsigned)kIndexed) + ")"); }
  { Req r; r.idx = r.o_pose = r.o_twist = r.o_acc = r.done_flag = r.done_count = true; PIN(kSepPacked, r, "(" + std::to_string((unsigned)kIndexed) + ")"); }
  { Req r; r.idx = true; r.gate_id_k = 3; PIN(kSepPacked, r, "(" + std::to_string((unsigned)kIndexed) + ")"); }   // gate_id 0: the other members are not read
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("update gate plan host test ok\n");
  return 0;
}
