// Host test of csrc/step_variant.hpp (no HIP): the rules of the step kernels' variant word and the launch plan of
// OpsImpl::step, over every request and every kind of OpsImpl the library has, plus the launch sequences of the requests the
// library serves today, pinned row by row.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/step_variant_host_test.cpp && ./a.out
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Req {
  bool idx = false, cls = false, rec_out = false, q_delta = false, pose = false, nis = false;
  bool o_pose = false, o_twist = false, o_acc = false, done_flag = false, done_count = false;
  bool live_posted = false, live_mirror = false, live_progress = false, live_done = false, live_pose = false;
  bool tile_uni = false, tile_blk = false;
  long live_ring = 0;
  int n_ticks = 1;
  long n = 65;
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

// the kinds of OpsImpl: {sep, shared, uniform_tiles, has_live, fused_pose_tick_by_tick, fused_spills, tpw}
static const StepTraits kSepFull{true, false, false, false, false, false, 64};       // LAYOUT_SEPARABLE
static const StepTraits kSepPacked{true, false, false, true, false, false, 64};      // LAYOUT_SEPARABLE_PACKED
static const StepTraits kSepPackedTbt{true, false, false, true, true, false, 64};    // ... angular_rates / uniform_acceleration fp32
static const StepTraits kShared{true, true, false, false, false, false, 64};         // LAYOUT_SEPARABLE_SHARED
static const StepTraits kSharedUt{true, true, true, false, false, false, 64};        // ... with uniform tiles
static const StepTraits kDense{false, false, false, false, false, false, 64};        // kf_step_kernel, thread per target
static const StepTraits kDenseG6{false, false, false, false, false, false, 10};      // ... 6 lanes per target
static const StepTraits kDenseSpills{false, false, false, false, false, true, 64};   // ... without a fused kernel
static const StepTraits* const kAllTraits[] = {&kSepFull, &kSepPacked, &kSepPackedTbt, &kShared, &kSharedUt, &kDense, &kDenseG6, &kDenseSpills};

// the launch sequence of a plan as text: "innov, 3 x (8 + pose)" -- the variant in decimal
static std::string show(const StepPlan& p, int n_ticks) {
  std::string s = p.innov_writer_first ? "innov, " : "";
  if (p.tick_by_tick) s += std::to_string(n_ticks) + " x ";
  return s + "(" + std::to_string(p.variant) + (p.pose_writer_after_each_tick ? " + pose)" : ")");
}
static std::string run(const StepTraits& t, const Req& r) {
  try {
    return show(plan_step(t, r), r.n_ticks);
  } catch (const std::runtime_error&) {
    return "throws";
  }
}
static std::string seq(unsigned v, bool pose_writer = false, int per_tick = 0, bool innov_first = false) {
  StepPlan p;
  p.variant = v; p.pose_writer_after_each_tick = pose_writer; p.tick_by_tick = per_tick > 0; p.innov_writer_first = innov_first;
  return show(p, per_tick);
}
#define PIN(traits, req, want) CHECK(run(traits, req) == (want), "%s, want %s", run(traits, req).c_str(), std::string(want).c_str())

static Req with(void (*f)(Req&)) { Req r; f(r); return r; }
static void make_live(Req& r) { r.live_posted = r.live_mirror = r.live_progress = r.live_done = true; r.live_ring = 8; r.n_ticks = 3; }
static void make_getters(Req& r) { r.idx = r.o_pose = r.o_twist = r.o_acc = r.done_flag = r.done_count = true; }

// Which GPU test launches each pinned row (found by logging every OpsImpl::step request and its plan over the GPU suite; the
// refused rows are stopped in Batch / Shard before they reach step and are pinned here only):
//   separable, one class
//     plain, idx, idx + o_pose      test_gpu_by_id.py::test_node_tick_sized_calls_by_id
//     3 ticks                       test_gpu_edge_cases.py::test_temporally_fused_launch_equals_single_ticks
//     q_delta                       test_gpu_intersection.py::test_all_batches_sequence_equals_per_batch_calls
//     rec_out                       test_gpu_mixed_configs.py::test_ab_ticks_forced_on_small_batches_match_oracle
//     pose, pose + 3 ticks (one launch, and tick by tick for fp32 angular_rates / uniform_acceleration on packed groups)
//                                   test_gpu_pose_stream.py::test_pose_stream_of_step_sequence_and_step_fused, ::test_ring_and_overwrite
//     pose + rec_out                test_gpu_pose_stream.py::test_poses_of_ab_and_zigzag_ticks_equal_in_place_ticks
//     pose + q_delta                test_gpu_shared_axes.py::test_by_id_erase_recreate_query_and_pose
//     nis                           test_gpu_innov_stream.py::test_innovations_of_every_layout
//     nis + pose                    test_gpu_innov_stream.py::test_with_poses_in_the_same_call
//     live                          test_gpu_live.py::test_live_session_equals_single_ticks_bit_for_bit
//     live + q_delta / live_pose    test_gpu_live.py::test_config4_share_resident_with_the_per_tick_query, ::test_per_tick_pose_output_of_a_live_session
//   separable, several classes
//     cls, cls + idx                test_gpu_classes.py::test_hundred_thousand_targets_thousand_classes_one_batch, ::test_one_at_a_time_inits_join_one_batch
//     cls + rec_out                 test_gpu_uniform_tiles.py::test_all_cases_with_forced_ab_ticks_and_zigzag
//     cls + 3 ticks                 test_gpu_classes.py::test_step_fused_on_a_batch_with_several_classes
//     cls + pose (+ 3 ticks)        test_gpu_pose_stream.py::test_fallback_layouts[classes-*]
//     cls + nis                     test_gpu_innov_stream.py::test_fallback_layouts[classes-*]
//     cls + nis + pose              test_gpu_innov_stream.py::test_several_classes_with_poses_in_the_same_call
//   shared form (with and without uniform tiles): plain, idx, q_delta, rec_out, pose, pose + q_delta, pose + rec_out, nis, nis + pose
//                                   test_gpu_shared_axes.py, test_gpu_uniform_tiles.py::test_launch_variants, test_gpu_innov_stream.py::test_shared_form_and_uniform_tiles
//   dense kernel
//     plain, idx, q_delta, rec_out  test_gpu_parity.py, test_gpu_intersection.py::test_all_batches_sequence_equals_per_batch_calls,
//                                   test_gpu_mixed_configs.py::test_ab_ticks_forced_on_small_batches_match_oracle
//     idx + o_pose                  test_gpu_edge_cases.py::test_getter_table_stays_current
//     cls, cls + idx                test_gpu_classes.py::test_coupled_classes_indexed_scalar_and_erase
//     cls + rec_out                 test_gpu_mixed_configs.py::test_ab_ticks_forced_on_a_dense_batch_with_several_classes_match_oracle
//     3 ticks, one launch           test_gpu_edge_cases.py::test_temporally_fused_launch_equals_single_ticks
//     3 ticks where fused_spills    test_gpu_edge_cases.py::test_fused_request_on_a_layout_without_a_fused_kernel
//     cls + 3 ticks                 test_gpu_classes.py::test_step_fused_on_a_batch_with_several_classes[uniform_acceleration-f64-True]
//     pose (+ 3 ticks)              test_gpu_pose_stream.py::test_fallback_layouts[coupled-*], ::test_pose_stream_of_step_sequence_and_step_fused
//     pose + rec_out                test_gpu_pose_stream.py::test_poses_of_ab_and_zigzag_ticks_equal_in_place_ticks
//     pose + q_delta                test_gpu_pose_stream.py::test_dense_layouts_with_poses_and_the_fused_query
//     nis, nis + pose               test_gpu_innov_stream.py::test_fallback_layouts[coupled-*], ::test_with_poses_in_the_same_call[angular_rates-f64-6]
static void pinned_rows() {
  // ---- separable layout, one class (every kind of separable OpsImpl unless the row names one)
  for (const StepTraits* t : {&kSepFull, &kSepPacked, &kSepPackedTbt, &kShared, &kSharedUt}) {
    PIN(*t, Req{}, seq(0));
    PIN(*t, with([](Req& r) { r.idx = true; }), seq(kIndexed));
    PIN(*t, with([](Req& r) { make_getters(r); }), seq(kIndexed));
    PIN(*t, with([](Req& r) { r.q_delta = true; }), seq(kQuery));
    PIN(*t, with([](Req& r) { r.rec_out = true; }), seq(kAB));
    PIN(*t, with([](Req& r) { r.pose = true; }), seq(kPose));
    PIN(*t, with([](Req& r) { r.pose = r.rec_out = true; }), seq(kAB | kPose));
    PIN(*t, with([](Req& r) { r.pose = r.q_delta = true; }), seq(kQuery | kPose));
    PIN(*t, with([](Req& r) { r.nis = true; }), seq(kInnov));
    PIN(*t, with([](Req& r) { r.nis = r.pose = true; }), seq(kInnov, true));
    PIN(*t, with([](Req& r) { r.nis = r.idx = true; }), "throws");
    PIN(*t, with([](Req& r) { make_getters(r); r.nis = true; }), "throws");
    PIN(*t, with([](Req& r) { r.nis = true; r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.nis = r.rec_out = true; }), "throws");
    PIN(*t, with([](Req& r) { r.nis = r.q_delta = true; }), "throws");
    PIN(*t, with([](Req& r) { r.rec_out = r.idx = true; }), "throws");
    PIN(*t, with([](Req& r) { r.rec_out = true; r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.rec_out = r.q_delta = true; }), "throws");
    if (!t->has_live) PIN(*t, with([](Req& r) { make_live(r); }), "throws");
  }
  for (const StepTraits* t : {&kSepFull, &kSepPacked, &kSepPackedTbt}) {
    PIN(*t, with([](Req& r) { r.n_ticks = 3; }), seq(kFused));
    PIN(*t, with([](Req& r) { r.pose = true; r.n_ticks = 3; }), t->fused_pose_tick_by_tick ? seq(kPose, false, 3) : seq(kFused | kPose));
  }
  for (const StepTraits* t : {&kSepPacked, &kSepPackedTbt}) {
    PIN(*t, with([](Req& r) { make_live(r); }), seq(kFused | kLive1));
    PIN(*t, with([](Req& r) { make_live(r); r.q_delta = true; }), seq(kFused | kLive2));
    PIN(*t, with([](Req& r) { make_live(r); r.live_pose = true; }), seq(kFused | kLive2));
  }
  // ---- separable layout, several classes
  for (const StepTraits* t : {&kSepFull, &kSepPacked, &kSepPackedTbt}) {
    PIN(*t, with([](Req& r) { r.cls = true; }), seq(kPerQR));
    PIN(*t, with([](Req& r) { r.cls = r.idx = true; }), seq(kIndexed | kPerQR));
    PIN(*t, with([](Req& r) { r.cls = r.rec_out = true; }), seq(kPerQR | kAB));
    PIN(*t, with([](Req& r) { r.cls = true; r.n_ticks = 3; }), seq(kPerQR, false, 3));
    PIN(*t, with([](Req& r) { r.cls = r.q_delta = true; }), "throws");
    PIN(*t, with([](Req& r) { r.cls = r.pose = true; }), seq(kPerQR, true));
    PIN(*t, with([](Req& r) { r.cls = r.pose = true; r.n_ticks = 3; }), seq(kPerQR, true, 3));
    PIN(*t, with([](Req& r) { r.cls = r.nis = true; }), seq(kPerQR, false, 0, true));
    PIN(*t, with([](Req& r) { r.cls = r.nis = r.pose = true; }), seq(kPerQR, true, 0, true));
  }
  // ---- shared form
  for (const StepTraits* t : {&kShared, &kSharedUt}) {
    PIN(*t, with([](Req& r) { r.cls = true; }), "throws");
    PIN(*t, with([](Req& r) { make_live(r); }), "throws");
    PIN(*t, with([](Req& r) { r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.tile_uni = r.tile_blk = true; }), t->uniform_tiles ? seq(0) : "throws");
    PIN(*t, with([](Req& r) { r.tile_uni = r.tile_blk = r.idx = true; }), "throws");
    PIN(*t, with([](Req& r) { r.tile_uni = true; }), "throws");
  }
  PIN(kSepPacked, with([](Req& r) { r.tile_uni = r.tile_blk = true; }), "throws");
  PIN(kDense, with([](Req& r) { r.tile_uni = r.tile_blk = true; }), "throws");
  // ---- dense kernel
  for (const StepTraits* t : {&kDense, &kDenseG6, &kDenseSpills}) {
    PIN(*t, Req{}, seq(0));
    PIN(*t, with([](Req& r) { r.idx = true; }), seq(kIndexed));
    PIN(*t, with([](Req& r) { r.q_delta = true; }), seq(kQuery));
    PIN(*t, with([](Req& r) { r.rec_out = true; }), seq(kAB));
    PIN(*t, with([](Req& r) { r.cls = true; }), seq(kPerQR));
    PIN(*t, with([](Req& r) { r.cls = r.idx = true; }), seq(kIndexed | kPerQR));
    PIN(*t, with([](Req& r) { r.cls = r.rec_out = true; }), seq(kPerQR | kAB));
    PIN(*t, with([](Req& r) { r.n_ticks = 3; }), t->fused_spills ? seq(0, false, 3) : seq(kFused));
    PIN(*t, with([](Req& r) { r.pose = true; }), seq(0, true));
    PIN(*t, with([](Req& r) { r.pose = true; r.n_ticks = 3; }), seq(0, true, 3));
    PIN(*t, with([](Req& r) { r.pose = r.q_delta = true; }), seq(kQuery, true));
    PIN(*t, with([](Req& r) { r.nis = true; }), seq(0, false, 0, true));
    PIN(*t, with([](Req& r) { make_live(r); }), "throws");
  }
  // a multi-tick request with the fused query or an A -> B destination is refused BEFORE the plan splits it into ticks, whichever
  // kernel would serve the ticks (where a fused kernel was missing, the code before the plan served these tick by tick: every tick
  // from the same source records)
  for (const StepTraits* t : kAllTraits) {
    PIN(*t, with([](Req& r) { r.q_delta = true; r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.pose = r.q_delta = true; r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.pose = r.rec_out = true; r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.cls = r.pose = r.rec_out = true; r.n_ticks = 3; }), "throws");
    PIN(*t, with([](Req& r) { r.cls = r.rec_out = true; r.n_ticks = 3; }), "throws");
  }
  // the getter table of an indexed launch: beyond one wavefront of entries it needs the wavefront counter
  PIN(kSepPacked, with([](Req& r) { make_getters(r); r.done_count = false; r.n = 64; }), seq(kIndexed));
  PIN(kSepPacked, with([](Req& r) { make_getters(r); r.done_count = false; r.n = 65; }), "throws");
  PIN(kDenseG6, with([](Req& r) { make_getters(r); r.done_count = false; r.n = 11; }), "throws");
  PIN(kSepPacked, with([](Req& r) { r.o_pose = r.o_twist = r.o_acc = r.done_flag = true; }), "throws");
}

// every request x every kind of OpsImpl: the plan throws, or names a kernel that exists
static long every_request() {
  long planned = 0;
  for (const StepTraits* t : kAllTraits)
    for (unsigned bits = 0; bits < (1u << 14); ++bits)
      for (int n_ticks : {1, 3}) {
        Req r;
        r.idx = bits & 1; r.cls = bits & 2; r.rec_out = bits & 4; r.q_delta = bits & 8; r.pose = bits & 16; r.nis = bits & 32;
        r.o_pose = bits & 64; r.o_twist = r.o_acc = r.done_flag = bits & 128; r.done_count = bits & 256;
        r.live_posted = bits & 512; r.live_mirror = r.live_progress = r.live_done = bits & 1024; r.live_ring = (bits & 1024) ? 8 : 0;
        r.live_pose = bits & 2048; r.tile_uni = bits & 4096; r.tile_blk = bits & 8192;
        r.n_ticks = n_ticks;
        StepPlan p;
        try {
          p = plan_step(*t, r);
        } catch (const std::runtime_error& e) {
          CHECK(std::string(e.what()).rfind("target_estimation_amd: ", 0) == 0, "%s", e.what());
          continue;
        }
        ++planned;
        const unsigned v = p.variant;
        CHECK(t->sep ? sep_variant_ok(v, t->shared) : dense_variant_ok(v), "request %u ticks %d: variant %u", bits, n_ticks, v);
        CHECK(variant_shipped(v, *t), "request %u ticks %d: variant %u is not shipped", bits, n_ticks, v);
        CHECK(t->sep ? variant_in(kSepVariants, v) : variant_in(kDenseVariants, v), "variant %u", v);
        CHECK(!p.tick_by_tick || n_ticks > 1, "request %u", bits);
        CHECK(!p.innov_writer_first || r.nis, "request %u", bits);
        CHECK(!p.pose_writer_after_each_tick || r.pose, "request %u", bits);
        if (sv_live(v)) {
          CHECK(r.live_posted && !p.tick_by_tick && !p.innov_writer_first && !p.pose_writer_after_each_tick, "request %u", bits);
          continue;
        }
        // every tick and both streams are served exactly once: by the kernel or by the launch around it
        CHECK(sv_has(v, kFused) == (n_ticks > 1 && !p.tick_by_tick), "request %u ticks %d variant %u", bits, n_ticks, v);
        CHECK((sv_has(v, kPose) || p.pose_writer_after_each_tick) == r.pose, "request %u variant %u", bits, v);
        CHECK(sv_has(v, kPose) != p.pose_writer_after_each_tick || !r.pose, "request %u variant %u", bits, v);
        CHECK((sv_has(v, kInnov) || p.innov_writer_first) == r.nis, "request %u variant %u", bits, v);
        CHECK(sv_has(v, kInnov) != p.innov_writer_first || !r.nis, "request %u variant %u", bits, v);
        CHECK(sv_has(v, kIndexed) == r.idx && sv_has(v, kQuery) == r.q_delta && sv_has(v, kPerQR) == r.cls && sv_has(v, kAB) == r.rec_out, "request %u variant %u", bits, v);
      }
  return planned;
}

int main() {
  // the rules themselves, where they are easy to get wrong
  static_assert(sep_variant_ok(kFused | kLive2, false) && !sep_variant_ok(kLive1, false) && !sep_variant_ok(kFused | kLiveMask, false), "live");
  static_assert(!sep_variant_ok(kFused, true) && !sep_variant_ok(kPerQR, true) && sep_variant_ok(kQuery | kPose, true), "shared form");
  static_assert(!dense_variant_ok(kPose) && !dense_variant_ok(kInnov) && !dense_variant_ok(kFused | kLive1) && dense_variant_ok(kPerQR | kAB), "dense");
  static_assert(!sep_variant_ok(kInnov | kPose, false) && !sep_variant_ok(kAB | kQuery, false) && !sep_variant_ok(1u << kVariantBits, false), "streams");
  static_assert(population_variant_ok(kAB | kPose, true) && !population_variant_ok(kIndexed, false) && !population_variant_ok(kQuery | kAB, false), "population");
  for (unsigned v : kSepVariants) CHECK(sep_variant_ok(v, false), "shipped separable variant %u", v);
  for (unsigned v : kDenseVariants) CHECK(dense_variant_ok(v), "shipped dense variant %u", v);
  pinned_rows();
  const long planned = every_request();
  std::printf("planned %ld requests\n", planned);
  CHECK(planned > 0, "nothing planned");
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("step variant host test ok\n");
  return 0;
}
