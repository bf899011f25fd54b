// CPU-only test of csrc/track_merge_plan.hpp, the HIP-free half of the duplicate-track search: the refusal table; the claim that a
// pair's reach2 never exceeds the larger of its two rows' reach2 (random Sigma and adversarial ones: equal, one ulp apart, 2^60
// apart, subnormal); the neighbour property for narrow pairs (random, on cell borders, one ulp either side, negative coordinates,
// at the clamp); d2 symmetry under the (lo, hi) order; the keyed pick under shuffled visiting orders with repeats; the classes and
// the survivor rule.  g++ alone, sanitised, contraction off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../target_estimation_amd/csrc/track_merge_plan.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

template <class F>
static bool refused(F&& f) {
  try { f(); } catch (const std::invalid_argument&) { return true; } catch (const std::runtime_error&) { return true; }
  return false;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static void good(const char* what, bool info, double dt, double gate, long rounds, double cell, long min_hits, long nb, bool per, long cap, bool ids) {
  CHECK(!refused([&] { te::check_merge_args(what, info, dt, gate, rounds, cell, min_hits, nb, per, cap, ids); }));
}
static void bad(bool info, double dt, double gate, long rounds, double cell, long min_hits, long nb, bool per, long cap, bool ids) {
  CHECK(refused([&] { te::check_merge_args("retire_duplicates", info, dt, gate, rounds, cell, min_hits, nb, per, cap, ids); }));
}

static void test_refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  good("find_duplicates", true, 0.01, 9.0, 4, 0.5, 1, 2, true, 0, true);
  good("find_duplicates", true, 0.0, 1e300, 1, 1e-300, 0, 0, false, 0, true);
  good("retire_duplicates", true, 0.01, 9.0, te::kAssocMaxRounds, 1e6, 255, 0, true, 0, false);
  good("retire_duplicates", true, 0.01, 9.0, 4, 0.5, 1, 0, true, 10, true);
  bad(false, 0.01, 9.0, 4, 0.5, 1, 2, true, 0, true);
  bad(true, -0.01, 9.0, 4, 0.5, 1, 2, true, 0, true);
  bad(true, nan, 9.0, 4, 0.5, 1, 2, true, 0, true);
  for (double gate : {0.0, -1.0, nan, inf, -inf}) bad(true, 0.01, gate, 4, 0.5, 1, 2, true, 0, true);
  for (double cell : {0.0, -1.0, nan, inf, -inf}) bad(true, 0.01, 9.0, 4, cell, 1, 2, true, 0, true);
  bad(true, 0.01, 9.0, 0, 0.5, 1, 2, true, 0, true);
  bad(true, 0.01, 9.0, te::kAssocMaxRounds + 1, 0.5, 1, 2, true, 0, true);
  bad(true, 0.01, 9.0, 4, 0.5, -1, 2, true, 0, true);
  bad(true, 0.01, 9.0, 4, 0.5, 256, 2, true, 0, true);
  bad(true, 0.01, 9.0, 4, 0.5, 1, -1, true, 0, true);
  bad(true, 0.01, 9.0, 4, 0.5, 1, 2, false, 0, true);
  bad(true, 0.01, 9.0, 4, 0.5, 1, 0, true, -1, true);
  bad(true, 0.01, 9.0, 4, 0.5, 1, 0, true, 5, false);
  CHECK(!refused([&] { te::check_merge_one_shard("find_duplicates", 1); }));
  CHECK(refused([&] { te::check_merge_one_shard("find_duplicates", 2); }));
}

// reach2 of a pair against the larger of its rows' reach2, on one axis
static void check_reach(double gate, double s_lo, double s_hi) {
  const double pair = te::assoc_grid_reach2(gate, s_lo + s_hi);
  const double r_lo = te::assoc_grid_reach2(gate, 2.0 * s_lo), r_hi = te::assoc_grid_reach2(gate, 2.0 * s_hi);
  CHECK(s_lo + s_hi <= 2.0 * std::max(s_lo, s_hi));
  CHECK(pair <= std::max(r_lo, r_hi));
}

static void test_pair_reach_claim() {
  const double gates[] = {1e-3, 0.75, 9.0, 16.0, 1e6};
  for (double gate : gates) {
    for (int t = 0; t < 20000; ++t) {
      const double a = std::ldexp(uniform() + 0.5, (int)(next_u64() % 80) - 40), b = std::ldexp(uniform() + 0.5, (int)(next_u64() % 80) - 40);
      check_reach(gate, a, b);
    }
    const double base[] = {1.0, 0.1, 1e-2, 3.0, 0.3333333333333333, 1e-300, 1e300 / 1e6};
    for (double s : base) {
      check_reach(gate, s, s);                                              // equal
      check_reach(gate, s, std::nextafter(s, 2.0 * s));                     // one ulp apart
      check_reach(gate, std::nextafter(s, 0.0), s);
      check_reach(gate, s, std::ldexp(s, -60));                             // 2^60 apart
      check_reach(gate, std::ldexp(s, -60), s);
    }
    const double den = std::numeric_limits<double>::denorm_min();
    check_reach(gate, den, den); check_reach(gate, den, 3.0 * den); check_reach(gate, 5.0 * den, 1e-310); check_reach(gate, 1e-310, 1.0);
  }
}

static void row_of(double* row, double x, double y, double z, double sxx, double syy, double szz) {
  row[0] = x; row[1] = y; row[2] = z;
  row[3] = sxx; row[4] = 0.0; row[5] = 0.0; row[6] = syy; row[7] = 0.0; row[8] = szz;
}

// two NARROW rows that pass the pair box lie within +-1 cell of each other on every axis
static void check_neighbours(double cell, double gate, const double* lo, const double* hi) {
  const double lim2 = te::assoc_grid_narrow_limit2(cell);
  if (te::merge_row_class(lo, 1, 1, gate, lim2) != te::kMergeEligible || te::merge_row_class(hi, 1, 1, gate, lim2) != te::kMergeEligible) return;
  double d2;
  if (!te::merge_pair_candidate(lo, hi, gate, &d2)) return;
  for (int a = 0; a < 3; ++a) {
    const int c0 = te::assoc_grid_coord(lo[a], cell), c1 = te::assoc_grid_coord(hi[a], cell);
    CHECK(std::abs(c0 - c1) <= 1);
  }
}

static long neighbour_cases = 0;
static void test_neighbour_property() {
  const double cells[] = {1e-3, 0.5, 1.0, 2.5, 1e3};
  for (double cell : cells) {
    const double gate = 9.0;
    const double s_narrow = cell * cell / (2.0 * gate) * 0.99;   // about the largest narrow Sigma_aa; the class itself decides
    for (int t = 0; t < 20000; ++t) {
      double lo[9], hi[9];
      const double s0 = s_narrow * (0.2 + 0.79 * uniform()), s1 = s_narrow * (0.2 + 0.79 * uniform());
      double base[3], other[3];
      for (int a = 0; a < 3; ++a) {
        const double k = std::floor((uniform() - 0.5) * 40.0);
        const int kind = (int)(next_u64() % 5);
        base[a] = kind == 0 ? k * cell : kind == 1 ? std::nextafter(k * cell, -1e300) : kind == 2 ? std::nextafter(k * cell, 1e300) : (k + uniform()) * cell;
        if (next_u64() % 16 == 0) base[a] += (next_u64() & 1 ? 1.0 : -1.0) * 1073741824.0 * cell;   // at the clamp
        other[a] = base[a] + (uniform() - 0.5) * 2.2 * cell;
      }
      row_of(lo, base[0], base[1], base[2], s0, s0 * (0.5 + uniform()), s0);
      row_of(hi, other[0], other[1], other[2], s1, s1, s1 * (0.5 + 0.5 * uniform()));
      double d2;
      if (te::merge_pair_candidate(lo, hi, gate, &d2)) ++neighbour_cases;
      check_neighbours(cell, gate, lo, hi);
      check_neighbours(cell, gate, hi, lo);
    }
  }
  CHECK(neighbour_cases > 1000);   // (the scenes do reach the claim)
}

static void test_d2_symmetry_and_invalid_sums() {
  for (int t = 0; t < 5000; ++t) {
    double r[2][10] = {};
    for (int i = 0; i < 2; ++i) {
      const double a = 0.01 + uniform(), b = 0.01 + uniform(), c = 0.01 + uniform();
      row_of(r[i], uniform(), uniform(), uniform(), a, b, c);
      r[i][4] = 0.3 * std::sqrt(a * b) * (uniform() - 0.5); r[i][7] = 0.3 * std::sqrt(b * c) * (uniform() - 0.5);
    }
    double all[20];
    std::memcpy(all, r[0], sizeof r[0]); std::memcpy(all + 10, r[1], sizeof r[1]);
    double d_a, d_b;
    const bool ok_a = te::merge_pair_candidate_of(all, 0, 1, 1e9, &d_a), ok_b = te::merge_pair_candidate_of(all, 1, 0, 1e9, &d_b);
    CHECK(ok_a == ok_b && std::memcmp(&d_a, &d_b, sizeof d_a) == 0);     // both partners: the same bits
    CHECK(ok_a && d_a >= 0.0);
  }
  // an indefinite sum rejects the pair; so does a NaN
  double lo[9], hi[9], d2;
  row_of(lo, 0, 0, 0, 0.75, 0.75, 0.75); lo[4] = 2.0;
  row_of(hi, 0.5, 0, 0, 0.75, 0.75, 0.75);
  CHECK(!te::merge_pair_candidate(lo, hi, 1e9, &d2) && d2 == -1.0);
  row_of(lo, 0, 0, 0, 0.75, 0.75, 0.75);
  CHECK(te::merge_pair_candidate(lo, hi, 1e9, &d2) && d2 == 0.25 / 1.5);
  hi[1] = std::numeric_limits<double>::quiet_NaN();
  CHECK(!te::merge_pair_candidate(lo, hi, 1e9, &d2));
  // d2 == gate is a candidate, one ulp below is not; the box alone can reject
  row_of(lo, 0, 0, 0, 0.5, 0.5, 0.5); row_of(hi, 3, 4, 0, 0.5, 0.5, 0.5);
  CHECK(te::merge_pair_candidate(lo, hi, 25.0, &d2) && d2 == 25.0);
  CHECK(!te::merge_pair_candidate(lo, hi, std::nextafter(25.0, 0.0), &d2));
  row_of(lo, 0, 0, 0, 1e-6, 1.0, 1.0); row_of(hi, 0, 0, 0, 1e-6, 1.0, 1.0);
  lo[4] = hi[4] = 0.0;
  CHECK(te::merge_pair_candidate(lo, hi, 4.0, &d2));
}

static void test_classes_and_survivor() {
  double row[9];
  const double lim2 = te::assoc_grid_narrow_limit2(0.5);
  row_of(row, 1, 2, 3, 0.01, 0.01, 0.01);
  CHECK(te::merge_row_class(row, 1, 1, 9.0, lim2) == te::kMergeEligible);
  CHECK(te::merge_row_class(row, 0, 1, 9.0, lim2) == te::kMergeNone);
  CHECK(te::merge_row_class(row, 0, 0, 9.0, lim2) == te::kMergeEligible);
  row[6] = 0.64;
  CHECK(te::merge_row_class(row, 5, 1, 9.0, lim2) == te::kMergeWide);
  CHECK(te::merge_row_class(row, 0, 1, 9.0, lim2) == te::kMergeNone);     // too few hits: not counted as wide either
  row[7] = std::numeric_limits<double>::infinity();
  CHECK(te::merge_row_class(row, 5, 1, 9.0, lim2) == te::kMergeNone);
  row[7] = 0.0; row[0] = std::numeric_limits<double>::quiet_NaN();
  CHECK(te::merge_row_class(row, 5, 1, 9.0, lim2) == te::kMergeNone);
  // the survivor: hits, then miss, then the row; exactly one of a pair is the weaker
  CHECK(te::merge_is_weaker(1, 0, 0, 2, 9, 1) && !te::merge_is_weaker(2, 9, 1, 1, 0, 0));
  CHECK(te::merge_is_weaker(2, 3, 0, 2, 1, 1) && !te::merge_is_weaker(2, 1, 1, 2, 3, 0));
  CHECK(te::merge_is_weaker(2, 1, 7, 2, 1, 3) && !te::merge_is_weaker(2, 1, 3, 2, 1, 7));
  for (int t = 0; t < 2000; ++t) {
    const int h0 = (int)(next_u64() % 3), h1 = (int)(next_u64() % 3), m0 = (int)(next_u64() % 3), m1 = (int)(next_u64() % 3);
    CHECK(te::merge_is_weaker(h0, m0, 4, h1, m1, 9) != te::merge_is_weaker(h1, m1, 9, h0, m0, 4));
  }
}

static void test_keyed_pick() {
  for (int t = 0; t < 500; ++t) {
    const int n = 1 + (int)(next_u64() % 20);
    std::vector<double> d2((size_t)n);
    for (double& v : d2) v = (double)(next_u64() % 4);            // few levels: ties
    int want = 0;
    for (int j = 1; j < n; ++j) if (d2[(size_t)j] < d2[(size_t)want]) want = j;
    std::vector<int> visit;
    for (int j = 0; j < n; ++j) for (uint64_t r = 0; r <= next_u64() % 3; ++r) visit.push_back(j);   // repeats
    for (size_t i = visit.size(); i > 1; --i) std::swap(visit[i - 1], visit[(size_t)(next_u64() % i)]);
    te::AssocBest best = te::assoc_best_none();
    for (int j : visit) te::assoc_take_keyed(best, d2[(size_t)j], j);
    CHECK(best.idx == want && best.d2 == d2[(size_t)want]);
  }
}

int main() {
  test_refusals();
  test_pair_reach_claim();
  test_neighbour_property();
  test_d2_symmetry_and_invalid_sums();
  test_classes_and_survivor();
  test_keyed_pick();
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("track merge plan host test ok\n");
  return 0;
}
