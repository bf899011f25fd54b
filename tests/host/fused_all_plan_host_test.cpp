// Host test of csrc/step_variant.hpp (no HIP): who serves a fused replay of a whole manager's shard (plan_fused_all), row by row;
// the predicate of the new launch (population_fused_ok) next to the ones it must not disturb; and the layout of the kernel's
// argument struct -- part k of PopulationFusedLayout lies at population_fused_seg_offset(k), which is what the gated loop of part k
// adds to the kernel-argument segment pointer.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/fused_all_plan_host_test.cpp && ./a.out
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../target_estimation_amd/csrc/dt_schedule.hpp"
#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

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

static const char* name(FusedAllRoute r) { return r == FusedAllRoute::kPerBatch ? "per batch" : r == FusedAllRoute::kPlainLoop ? "plain loop" : "gated loop"; }
static FusedAllRoute plan(const std::vector<FusedAllBatch>& b, bool scheduled = false, long n_ticks = 7, bool population_tick = true, bool f64 = true) {
  return plan_fused_all(population_tick, f64, b.data(), (long)b.size(), scheduled, n_ticks, kDtTabMaxTicks);
}
#define PIN(got, want) CHECK((got) == (want), "%s, want %s", name(got), name(want))

static FusedAllBatch batch(int type, long n = 65) {
  FusedAllBatch b;
  b.n = n; b.type = type; b.ready = true;
  return b;
}
static FusedAllBatch with_nis(FusedAllBatch b, bool gate = true) { b.nis = true; b.gate_or_policy = gate; return b; }

// stand-ins for FusedGateDtSegment<double> / <float>: what matters is that the parts are an array at the head of the struct
struct SegA { char a[408]; double g[14]; const double* tab; };
struct SegB { int a[3]; double g; };
struct SegHuge { char a[1200]; };

int main() {
  const FusedAllRoute per = FusedAllRoute::kPerBatch, plain = FusedAllRoute::kPlainLoop, gated = FusedAllRoute::kGatedLoop;
  // ---- the predicates: the new one is stated on its own, the old ones answer as they did
  static_assert(population_fused_ok(true, false, false) && population_fused_ok(true, true, true) && population_fused_ok(false, true, false) &&
                    population_fused_ok(false, false, true), "every instantiation is shipped");
  static_assert(!population_variant_ok(kFused, false) && !population_variant_ok(kFused | kInnov, false) && population_variant_ok(kInnov, true),
                "the single-tick population kernel's predicate does not know the fused launch");
  static_assert(sep_variant_ok(kFused, false) && !sep_variant_ok(kFused, true) && !sep_variant_ok(kFused | kInnov, false), "sep_variant_ok as it was");
  static_assert(kVariantBits == 9, "no new bit in the variant word");
  // ---- one launch: the plain loop
  PIN(plan({batch(0), batch(1), batch(2), batch(3)}), plain);
  PIN(plan({batch(3, 130), batch(0), batch(2, 1), batch(1, 64)}), plain);   // batch order is not part order
  PIN(plan({batch(2), batch(0)}), plain);                                  // an absent model in the middle
  PIN(plan({batch(2), batch(1, 0), batch(0)}), plain);                     // an empty batch takes no part
  PIN(plan({batch(0), batch(3)}, true, 1), plain);                         // a schedule, one tick
  PIN(plan({batch(0), batch(3)}, true, kDtTabMaxTicks), plain);
  PIN(plan({batch(0), batch(3)}, false, kDtTabMaxTicks + 1), plain);       // (the limit is the table's)
  PIN(plan({batch(0), batch(3)}, false, 7, true, false), plain);           // fp32
  // ---- one launch: the gated loop -- every non-empty batch has at least its NIS rows
  PIN(plan({with_nis(batch(0)), with_nis(batch(1)), with_nis(batch(2)), with_nis(batch(3))}), gated);
  PIN(plan({with_nis(batch(0)), with_nis(batch(3), false)}), gated);       // nis_max 0 on one batch: its plain stream
  PIN(plan({with_nis(batch(0), false), with_nis(batch(3), false)}), gated);
  PIN(plan({with_nis(batch(0)), batch(1, 0), with_nis(batch(3))}, true), gated);   // (an empty batch needs no rows)
  // ---- per batch inside the call
  PIN(plan({}), per);
  PIN(plan({batch(0)}), per);                                              // a single non-empty batch
  PIN(plan({batch(0), batch(1, 0)}), per);
  PIN(plan({batch(0), batch(0)}), per);                                    // two batches of one model (two layouts)
  PIN(plan({batch(0), batch(4)}), per);
  { auto b = batch(1); b.ready = false; PIN(plan({batch(0), b}), per); }   // coupled or dense layouts, several (Q, R) classes
  { auto b = batch(1); b.keep_meas = true; PIN(plan({batch(0), b}), per); }
  { auto b = batch(1); b.pose = true; PIN(plan({batch(0), b}), per); PIN(plan({with_nis(batch(0)), with_nis(b)}), per); }
  PIN(plan({with_nis(batch(0)), batch(3)}), per);                          // only some batches carry streams
  PIN(plan({with_nis(batch(0), false), batch(3)}), per);
  PIN(plan({batch(0), batch(3)}, true, kDtTabMaxTicks + 1), per);          // a schedule beyond one table
  PIN(plan({with_nis(batch(0)), with_nis(batch(3))}, true, kDtTabMaxTicks + 1), per);
  PIN(plan({batch(0), batch(3)}, false, 7, false), per);                   // ShardSettings::population_tick off
  // ---- the argument struct: part k at population_fused_seg_offset(k), the grid split behind the parts, 4 KB at most
#define AT(Seg, k) CHECK(offsetof(PopulationFusedLayout<Seg>, part[k]) == population_fused_seg_offset<Seg>(k), "%zu, %u", offsetof(PopulationFusedLayout<Seg>, part[k]), population_fused_seg_offset<Seg>(k))
  AT(SegA, 0); AT(SegA, 1); AT(SegA, 2); AT(SegA, 3);
  AT(SegB, 0); AT(SegB, 1); AT(SegB, 2); AT(SegB, 3);
  static_assert(population_fused_seg_offset<SegA>(0) == 0 && offsetof(PopulationFusedLayout<SegA>, part) == 0, "the per-batch kernels' offset");
  CHECK(offsetof(PopulationFusedLayout<SegA>, end) == 4 * sizeof(SegA) && offsetof(PopulationFusedLayout<SegB>, end) == 4 * sizeof(SegB), "end[4] behind the parts");
  static_assert(population_fused_args_fit<SegA>() && population_fused_args_fit<SegB>() && !population_fused_args_fit<SegHuge>(), "the 4 KB limit");
  std::printf(g_fail ? "FUSED ALL PLAN HOST TEST FAILED (%d)\n" : "fused all plan host test ok\n", g_fail);
  return g_fail ? 1 : 0;
}
