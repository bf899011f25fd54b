// The HIP-free half of the track lifecycle (csrc/lifecycle_plan.hpp), g++ alone: the refusal table, the counters, the stale and
// finiteness rules, the block cover for awkward sizes, the ordered compaction's block arithmetic against a sequential pass, the
// id-range wrap check.
#include "../../target_estimation_amd/csrc/lifecycle_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace te;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool refused(const LifecyclePolicy* p, bool info, long M, bool det, bool sod, long nb, bool masks, long cap, bool ret, const char* why) {
  try {
    check_lifecycle_args(p, info, M, det, sod, nb, masks, cap, ret);
  } catch (const std::invalid_argument& e) {
    const bool ok = std::string(e.what()).find(why) != std::string::npos;
    if (!ok) std::printf("refused with '%s', expected '%s'\n", e.what(), why);
    return ok;
  }
  std::printf("not refused: %s\n", why);
  return false;
}

// the compaction as the three kernels do it, on the host: per block the count, the exclusive scan of the counts, rank = block
// offset + waves before + lanes below
static std::vector<int> compact_blocks(const std::vector<unsigned char>& flag, unsigned char want) {
  const long n = (long)flag.size(), nb = n > 0 ? lifecycle_blocks(n) : 0;
  std::vector<int> sums((size_t)nb, 0), out;
  std::vector<unsigned long long> ballots((size_t)nb * kLifecycleWaves, 0ull);
  for (long i = 0; i < n; ++i)
    if (flag[(size_t)i] == want) { ballots[(size_t)(i / 64)] |= 1ull << (i % 64); ++sums[(size_t)(i / kLifecycleThreads)]; }
  int carry = 0;
  for (long b = 0; b < nb; ++b) { const int v = sums[(size_t)b]; sums[(size_t)b] = carry; carry += v; }
  out.assign((size_t)carry, -1);
  for (long i = 0; i < n; ++i) {
    if (flag[(size_t)i] != want) continue;
    const long blk = i / kLifecycleThreads;
    const int tid = (int)(i % kLifecycleThreads), wave = tid / 64, lane = tid % 64;
    int before = 0;
    for (int w = 0; w < wave; ++w) before += __builtin_popcountll(ballots[(size_t)(blk * kLifecycleWaves + w)]);
    const int pos = sums[(size_t)blk] + before + lifecycle_rank_in_wave(ballots[(size_t)(blk * kLifecycleWaves + wave)], lane);
    CHECK(pos >= 0 && pos < carry && out[(size_t)pos] == -1);
    if (pos >= 0 && pos < carry) out[(size_t)pos] = (int)i;
  }
  return out;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- the refusal table
  LifecyclePolicy good;
  good.max_misses = 3; good.birth_type = 3; good.first_id = 10; good.max_births = 5; good.dt0 = 0.01; good.t_birth = 1.0;
  try { check_lifecycle_args(&good, true, 8, true, true, 2, true, 4, true); } catch (...) { CHECK(!"a good call was refused"); }
  try { check_lifecycle_args(&good, true, 0, false, false, 0, false, 0, false); } catch (...) { CHECK(!"an empty call was refused"); }
  CHECK(refused(nullptr, true, 8, true, true, 2, true, 4, true, "policy is required"));
  CHECK(refused(&good, false, 8, true, true, 2, true, 4, true, "info is required"));
  CHECK(refused(&good, true, -1, true, true, 2, true, 4, true, "M must be 0..1048576"));
  CHECK(refused(&good, true, kLifecycleMaxDetections + 1, true, true, 2, true, 4, true, "M must be 0..1048576"));
  try { check_lifecycle_args(&good, true, kLifecycleMaxDetections, true, true, 2, true, 4, true); } catch (...) { CHECK(!"M at the limit was refused"); }
  { LifecyclePolicy p = good; p.max_misses = -1; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "max_misses must be 0..255")); }
  { LifecyclePolicy p = good; p.max_misses = 256; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "max_misses must be 0..255")); }
  { LifecyclePolicy p = good; p.birth_type = -2; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "birth_type must be -1..3")); }
  { LifecyclePolicy p = good; p.birth_type = 4; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "birth_type must be -1..3")); }
  { LifecyclePolicy p = good; p.max_births = -1; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "max_births must be >= 0")); }
  { LifecyclePolicy p = good; p.t_birth = nan; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "must not be NaN")); }
  { LifecyclePolicy p = good; p.dt0 = nan; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "must not be NaN")); }
  { const double q = 1.0; LifecyclePolicy p = good; p.Q = &q; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "together or not at all")); }
  { const double q = 1.0; LifecyclePolicy p = good; p.R = &q; p.P0 = &q; CHECK(refused(&p, true, 8, true, true, 2, true, 4, true, "together or not at all")); }
  CHECK(refused(&good, true, 8, false, true, 2, true, 4, true, "required for births"));
  CHECK(refused(&good, true, 8, true, false, 2, true, 4, true, "required for births"));
  { LifecyclePolicy p = good; p.birth_type = -1;   // no births: the frame is not needed
    try { check_lifecycle_args(&p, true, 8, false, false, 2, true, 4, true); } catch (...) { CHECK(!"the retirement half was refused"); } }
  CHECK(refused(&good, true, 8, true, true, -1, true, 4, true, "one mask per batch"));
  CHECK(refused(&good, true, 8, true, true, 2, false, 4, true, "one mask per batch"));
  CHECK(refused(&good, true, 8, true, true, 2, true, -1, true, "retired_ids_out"));
  CHECK(refused(&good, true, 8, true, true, 2, true, 4, false, "retired_ids_out"));

  // ---- the counters
  { unsigned char m = 0, h = 0;
    for (int k = 0; k < 300; ++k) lifecycle_count(0, m, h);
    CHECK(m == 255 && h == 0);
    lifecycle_count(1, m, h);
    CHECK(m == 0 && h == 1);
    for (int k = 0; k < 300; ++k) lifecycle_count(7, m, h);   // any non-zero byte is a match
    CHECK(m == 0 && h == 255);
    lifecycle_count(0, m, h);
    CHECK(m == 1 && h == 255); }
  CHECK(!lifecycle_stale(0, 255) && !lifecycle_stale(3, 2) && lifecycle_stale(3, 3) && lifecycle_stale(1, 1) && !lifecycle_stale(1, 0));
  CHECK(lifecycle_stale(255, 255) && !lifecycle_stale(255, 254));

  // ---- finiteness and the detection flag
  { double row[7] = {1, 2, 3, 0, 0, 0, 1};
    CHECK(lifecycle_row_finite(row) && lifecycle_det_flag(-1, row) == kLifecycleDetCandidate && lifecycle_det_flag(5, row) == kLifecycleDetMatched);
    for (int c = 0; c < 7; ++c)
      for (double bad : {nan, inf, -inf}) {
        double r2[7]; for (int k = 0; k < 7; ++k) r2[k] = row[k];
        r2[c] = bad;
        CHECK(!lifecycle_row_finite(r2) && lifecycle_det_flag(-1, r2) == kLifecycleDetNonFinite && lifecycle_det_flag(0, r2) == kLifecycleDetMatched);
      } }

  // ---- the block cover
  for (long n : {0L, 1L, 63L, 64L, 65L, 255L, 256L, 257L, 1025L, 1000000L, 1048576L}) {
    const long b = lifecycle_blocks(n);
    CHECK(b >= 1 && b * kLifecycleThreads >= n && (n <= kLifecycleThreads || (b - 1) * kLifecycleThreads < n));
  }
  // ---- the rank inside a wavefront
  CHECK(lifecycle_rank_in_wave(~0ull, 0) == 0 && lifecycle_rank_in_wave(~0ull, 63) == 63 && lifecycle_rank_in_wave(1ull << 63, 63) == 0);
  CHECK(lifecycle_rank_in_wave(0x5ull, 2) == 1 && lifecycle_rank_in_wave(0x5ull, 3) == 2 && lifecycle_rank_in_wave(0ull, 40) == 0);

  // ---- the compaction against a sequential pass
  std::srand(11);
  for (long n : {0L, 1L, 63L, 64L, 65L, 255L, 256L, 257L, 300L, 1025L, 70000L}) {
    for (int density : {0, 1, 2, 50, 100}) {
      std::vector<unsigned char> flag((size_t)n);
      for (auto& f : flag) { const int r = std::rand() % 100; f = r < density ? 1 : (r % 3 == 0 ? 2 : 0); }
      for (unsigned char want : {(unsigned char)1, (unsigned char)2}) {
        std::vector<int> seq;
        for (long i = 0; i < n; ++i) if (flag[(size_t)i] == want) seq.push_back((int)i);
        CHECK(compact_blocks(flag, want) == seq);
      }
    }
  }
  CHECK(lifecycle_born(300, 257) == 257 && lifecycle_born(3, 257) == 3 && lifecycle_born(5, 0) == 0);

  // ---- the id range
  CHECK(!lifecycle_ids_wrap(0xFFFFFFFFu, 0) && !lifecycle_ids_wrap(0xFFFFFFFFu, 1) && lifecycle_ids_wrap(0xFFFFFFFFu, 2));
  CHECK(!lifecycle_ids_wrap(0u, 1048576) && lifecycle_ids_wrap(0xFFF00000u, 1048577) && !lifecycle_ids_wrap(0xFFF00000u, 1048576));

  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("lifecycle plan host test ok\n");
  return 0;
}
