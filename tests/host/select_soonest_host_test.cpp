// CPU only (g++ -fsanitize=address,undefined): the HIP-free half of the k-soonest selection, csrc/select_soonest_plan.hpp --
// the key and its order, the filler row, the argument checks as a table, the first stage's grid, and the merge of the shards'
// rows against a brute-force sort.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../target_estimation_amd/csrc/select_soonest_plan.hpp"

using namespace te;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static bool refused(long k, double lo, double hi, bool delta, bool pose, bool pose_out, bool outputs) {
  try { check_soonest_args(k, lo, hi, delta, pose, pose_out, outputs); } catch (const std::invalid_argument&) { return true; }
  return false;
}

static void test_key_order() {
  const double inf = std::numeric_limits<double>::infinity();
  // the bits of non-negative doubles order as the doubles do
  const double v[] = {0.0, 4.9e-324, 1e-300, 0.5, 1.0, 1.0000000000000002, 3.5, 1e300, inf};
  for (size_t i = 0; i + 1 < sizeof v / sizeof v[0]; ++i) {
    CHECK(soonest_key_less(soonest_key(v[i], 0, 0), soonest_key(v[i + 1], 0, 0)));
    CHECK(!soonest_key_less(soonest_key(v[i + 1], 0, 0), soonest_key(v[i], 0, 0)));
  }
  // -0.0 == 0.0: the slot decides, whichever of the two zeros a slot holds
  CHECK(soonest_delta_bits(-0.0) == soonest_delta_bits(0.0));
  CHECK(soonest_key_less(soonest_key(0.0, 0, 3), soonest_key(-0.0, 0, 4)));
  CHECK(soonest_key_less(soonest_key(-0.0, 0, 3), soonest_key(0.0, 0, 4)));
  // ties: batch, then slot
  CHECK(soonest_key_less(soonest_key(2.0, 0, 9), soonest_key(2.0, 1, 0)));
  CHECK(soonest_key_less(soonest_key(2.0, 1, 0), soonest_key(2.0, 1, 1)));
  CHECK(!soonest_key_less(soonest_key(2.0, 1, 1), soonest_key(2.0, 1, 1)));
  // delta before batch
  CHECK(soonest_key_less(soonest_key(1.0, 7, 7), soonest_key(2.0, 0, 0)));
  // the empty row is above every candidate, +inf included
  CHECK(soonest_key_less(soonest_key(inf, 0x7fffffff, 0x7fffffff), soonest_key_none()));
  CHECK(soonest_key_is_none(soonest_key_none()) && !soonest_key_is_none(soonest_key(inf, 0, 0)));
  const SoonestKey k = soonest_key(1.5, 12, 345678);
  CHECK(soonest_key_batch(k) == 12 && soonest_key_slot(k) == 345678);
  // the candidate rule
  const double nan = std::nan("");
  CHECK(soonest_candidate(0.0, true, 0.0, inf) && soonest_candidate(-0.0, true, 0.0, inf) && soonest_candidate(inf, true, 0.0, inf));
  CHECK(!soonest_candidate(-1.0, true, 0.0, inf) && !soonest_candidate(nan, true, 0.0, inf) && !soonest_candidate(1.0, false, 0.0, inf));
  CHECK(soonest_candidate(1.0, true, 1.0, 2.0) && soonest_candidate(2.0, true, 1.0, 2.0) && !soonest_candidate(2.0000000000000004, true, 1.0, 2.0));
  // the filler is what no_intersection writes
  const SoonestRow f = soonest_filler();
  CHECK(f.batch == -1 && f.slot == -1 && f.delta == -1.0 && f.pose[6] == 1.0);
  for (int c = 0; c < 6; ++c) CHECK(f.pose[c] == 0.0);
  // rows order as keys do
  SoonestRow a, b;
  a.delta = -0.0; a.batch = 0; a.slot = 5; b.delta = 0.0; b.batch = 0; b.slot = 6;
  CHECK(soonest_row_less(a, b) && !soonest_row_less(b, a));
}

static void test_checks() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  struct Case { long k; double lo, hi; bool delta, pose, pose_out, outputs; bool refused; };
  const Case table[] = {
      {8, 0.0, inf, true, false, false, true, false},
      {1, 0.0, 0.0, true, true, true, true, false},
      {256, 1.0, 2.0, true, true, true, true, false},
      {0, 0.0, inf, true, false, false, true, true},      // k out of range
      {257, 0.0, inf, true, false, false, true, true},
      {-1, 0.0, inf, true, false, false, true, true},
      {8, -1.0, inf, true, false, false, true, true},     // delta_lo < 0
      {8, -1e-300, inf, true, false, false, true, true},
      {8, nan, inf, true, false, false, true, true},      // NaN window
      {8, 0.0, nan, true, false, false, true, true},
      {8, 2.0, 1.0, true, false, false, true, true},      // delta_hi < delta_lo
      {8, inf, inf, true, false, false, true, false},     // (an empty-looking but valid window)
      {8, 0.0, inf, false, false, false, true, true},     // NULL delta
      {8, 0.0, inf, true, false, false, false, true},     // a NULL output
      {8, 0.0, inf, true, false, true, true, true},       // pose_out without pose
      {8, 0.0, inf, true, true, false, true, true},       // pose without pose_out
  };
  for (const Case& c : table) CHECK(refused(c.k, c.lo, c.hi, c.delta, c.pose, c.pose_out, c.outputs) == c.refused);
  // more batches of one device than a launch's arguments hold
  for (long parts = 0; parts <= kSoonestMaxParts + 2; ++parts) {
    bool thrown = false;
    try { check_soonest_parts(parts); } catch (const std::invalid_argument&) { thrown = true; }
    CHECK(thrown == (parts > kSoonestMaxParts));
  }
  CHECK(soonest_max_wgs_from(nullptr) == kSoonestDefaultMaxWgs && soonest_max_wgs_from("") == kSoonestDefaultMaxWgs);
  CHECK(soonest_max_wgs_from("3") == 3 && soonest_max_wgs_from("0") == 1 && soonest_max_wgs_from("x") == kSoonestDefaultMaxWgs);
  CHECK(soonest_max_wgs_from("99999999") == kSoonestMaxWgsLimit);
}

static void test_grid() {
  int wb[kSoonestMaxParts + 1];
  {  // one chunk per workgroup while the cap allows
    const long n[] = {1000, 0, 257};
    const int g = plan_soonest_grid(n, 3, 1024, wb);
    CHECK(g == 6 && wb[0] == 0 && wb[1] == 4 && wb[2] == 4 && wb[3] == 6);
  }
  {  // capped: shares, at least one per part with entries, never more than a part's chunks
    const long n[] = {100000, 1, 50000};
    const int g = plan_soonest_grid(n, 3, 8, wb);
    CHECK(wb[1] - wb[0] >= 1 && wb[2] - wb[1] == 1 && wb[3] - wb[2] >= 1 && g == wb[3] && g <= 8 + 3);
  }
  {  // every chunk is covered exactly once by the strided walk
    std::mt19937 rng(1);
    for (int it = 0; it < 200; ++it) {
      long n[4];
      const int parts = 1 + (int)(rng() % 4);
      for (int p = 0; p < parts; ++p) n[p] = (long)(rng() % 5000);
      const int cap = 1 + (int)(rng() % 12);
      const int g = plan_soonest_grid(n, parts, cap, wb);
      CHECK(g >= 1 && g <= cap + parts);
      for (int p = 0; p < parts; ++p) {
        const long chunks = (n[p] + kSoonestChunk - 1) / kSoonestChunk;
        const int w = wb[p + 1] - wb[p];
        CHECK(chunks == 0 ? w == 0 : (w >= 1 && w <= chunks));
        std::vector<int> seen((size_t)chunks, 0);
        for (int j = 0; j < w; ++j) {
          const long rounds = j < chunks ? (chunks - j + w - 1) / w : 0;
          for (long r = 0; r < rounds; ++r) { CHECK(j + r * w < chunks); if (j + r * w < chunks) ++seen[(size_t)(j + r * w)]; }
        }
        for (int s : seen) CHECK(s == 1);
      }
    }
  }
  {  // a small call keeps to one middle workgroup's lists: 10 000 entries are 40 chunks on 32 workgroups; a larger one does not
    const long n[] = {10000};
    CHECK(plan_soonest_grid(n, 1, 1024, wb) == 32);
    const long m[] = {256 * 65};
    CHECK(plan_soonest_grid(m, 1, 1024, wb) == 65);
  }
  {  // nothing at all still runs one workgroup
    const long n[] = {0};
    CHECK(plan_soonest_grid(n, 1, 1024, wb) == 1 && wb[1] == 0);
    CHECK(plan_soonest_grid(n, 0, 1024, wb) == 1);
  }
  CHECK(soonest_mid_wgs(1) == 1 && soonest_mid_wgs(32) == 1 && soonest_mid_wgs(33) == 2);
  CHECK(soonest_scratch_rows(33) == (size_t)(33 + 2) * 256);
}

static void test_merge() {
  std::mt19937 rng(7);
  for (int it = 0; it < 300; ++it) {
    const int shards = 1 + (int)(rng() % 4);
    const long k = 1 + (long)(rng() % 20);
    const bool tied = it % 2 == 0;   // heavily tied: deltas from a set of three values, -0.0 among them
    std::vector<std::vector<SoonestRow>> per((size_t)shards);
    std::vector<SoonestRow> all;
    int batch = 0;
    for (int s = 0; s < shards; ++s) {
      std::vector<SoonestRow> mine;
      const int batches = 1 + (int)(rng() % 2);
      for (int b = 0; b < batches; ++b, ++batch) {
        const int n = (int)(rng() % 30);   // often fewer than k
        for (int i = 0; i < n; ++i) {
          SoonestRow r;
          r.batch = batch; r.slot = i;
          const double three[] = {-0.0, 0.0, 1.25};
          r.delta = tied ? three[rng() % 3] : (double)(rng() % 1000) / 8.0;
          r.pose[0] = (double)(batch * 1000 + i);
          mine.push_back(r);
        }
      }
      std::sort(mine.begin(), mine.end(), soonest_row_less);
      all.insert(all.end(), mine.begin(), mine.end());
      if ((long)mine.size() > k) mine.resize((size_t)k);   // a shard hands in its k best at most
      per[(size_t)s] = mine;
    }
    std::stable_sort(all.begin(), all.end(), soonest_row_less);
    std::vector<SoonestRow> out((size_t)k);
    const long count = merge_soonest(per, k, out.data());
    CHECK(count == std::min<long>(k, (long)all.size()));
    for (long i = 0; i < k; ++i) {
      if (i < count) {
        CHECK(out[(size_t)i].batch == all[(size_t)i].batch && out[(size_t)i].slot == all[(size_t)i].slot);
        CHECK(std::signbit(out[(size_t)i].delta) == std::signbit(all[(size_t)i].delta) && out[(size_t)i].delta == all[(size_t)i].delta);
        CHECK(out[(size_t)i].pose[0] == all[(size_t)i].pose[0]);
      } else {
        CHECK(out[(size_t)i].batch == -1 && out[(size_t)i].slot == -1 && out[(size_t)i].delta == -1.0 && out[(size_t)i].pose[6] == 1.0);
      }
    }
  }
}

int main() {
  test_key_order();
  test_checks();
  test_grid();
  test_merge();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("select soonest host test ok\n");
  return 0;
}
