// CPU-only test of csrc/associate_grid_plan.hpp, the HIP-free half of the grid form of the association: the refusal table, the
// bucket-count plan with forced values, the neighbour property of the cell map (for a narrow reach2 every x inside the box lands
// within +-1 cell of zhat: random inputs and adversarial ones -- borders, one ulp either side, negative coordinates, the clamp at
// +-2^30 cells, cell from 1e-3 to 1e3), the box against the gate, and the keyed pick against a sorted pass under shuffled visiting
// orders with ties and repeats.  g++ alone, sanitised, contraction off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../target_estimation_amd/csrc/associate_grid_plan.hpp"

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

static void test_refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(!refused([&] { te::check_assoc_grid_args(0.01, true, 10, 9.0, 4, 0.5, true, 16, 16); }));
  CHECK(!refused([&] { te::check_assoc_grid_args(0.0, true, te::kAssocGridMaxDetections, 1e300, 1, 1e-300, true, 16, 10); }));
  CHECK(!refused([&] { te::check_assoc_grid_args(0.01, false, 0, 9.0, te::kAssocMaxRounds, 1e6, true, 0, 0); }));
  CHECK(te::kAssocGridMaxDetections == 1048576 && te::kAssocGridMaxDetections > te::kAssocMaxDetections);
  CHECK(refused([&] { te::check_assoc_grid_args(-0.01, true, 10, 9.0, 4, 0.5, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(nan, true, 10, 9.0, 4, 0.5, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, -1, 9.0, 4, 0.5, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, te::kAssocGridMaxDetections + 1, 9.0, 4, 0.5, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, false, 3, 9.0, 4, 0.5, true, 16, 16); }));
  for (double gate : {0.0, -1.0, nan, inf, -inf}) CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, 10, gate, 4, 0.5, true, 16, 16); }));
  for (double cell : {0.0, -1.0, nan, inf, -inf}) CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, 10, 9.0, 4, cell, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, 10, 9.0, 0, 0.5, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, 10, 9.0, te::kAssocMaxRounds + 1, 0.5, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, 10, 9.0, 4, 0.5, false, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_grid_args(0.01, true, 10, 9.0, 4, 0.5, true, 15, 16); }));
  // the switch of the entry points that serve both forms: cell 0 is the brute-force form with ITS rules
  CHECK(!refused([&] { te::check_assoc_args_for(0.0, 0.01, true, 10, inf, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args_for(0.5, 0.01, true, 10, inf, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args_for(0.0, 0.01, true, te::kAssocMaxDetections + 1, 9.0, 4, true, 16, 16); }));
  CHECK(!refused([&] { te::check_assoc_args_for(0.5, 0.01, true, te::kAssocMaxDetections + 1, 9.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args_for(nan, 0.01, true, 10, 9.0, 4, true, 16, 16); }));
}

static void test_buckets() {
  CHECK(te::plan_assoc_grid_buckets(0, 0) == 1024 && te::plan_assoc_grid_buckets(512, 0) == 1024 && te::plan_assoc_grid_buckets(513, 0) == 2048);
  CHECK(te::plan_assoc_grid_buckets(1000000, 0) == (1L << 21) && te::plan_assoc_grid_buckets(1048576, 0) == (1L << 21));
  for (long c : {1L, 7L, 1023L, 4097L, 99999L, 1048576L, 5000000L}) {
    const long h = te::plan_assoc_grid_buckets(c, 0);
    CHECK(h >= 1024 && h >= 2 * c && (h & (h - 1)) == 0 && (h == 1024 || h / 2 < 2 * c));
  }
  CHECK(te::plan_assoc_grid_buckets(1000000, 1) == 1 && te::plan_assoc_grid_buckets(5, 4) == 4);
  CHECK(te::assoc_grid_forced_buckets_from(nullptr) == 0 && te::assoc_grid_forced_buckets_from("") == 0 && te::assoc_grid_forced_buckets_from("x") == 0);
  CHECK(te::assoc_grid_forced_buckets_from("0") == 0 && te::assoc_grid_forced_buckets_from("-4") == 0);
  CHECK(te::assoc_grid_forced_buckets_from("1") == 1 && te::assoc_grid_forced_buckets_from("4") == 4 && te::assoc_grid_forced_buckets_from("5") == 4);
  CHECK(te::assoc_grid_forced_buckets_from("99999999999") == te::kAssocGridMaxBuckets);
  // the hash stays inside the mask and spreads neighbouring cells
  std::vector<int> seen(1024, 0);
  for (int x = -8; x < 8; ++x)
    for (int y = -8; y < 8; ++y)
      for (int z = -2; z < 2; ++z) {
        const unsigned b = te::assoc_grid_hash(x, y, z, 1023u);
        CHECK(b < 1024u);
        seen[b]++;
        CHECK(te::assoc_grid_hash(x, y, z, 0u) == 0u);
      }
  int used = 0, most = 0;
  for (int c : seen) { used += c > 0; most = std::max(most, c); }
  CHECK(used > 500 && most <= 8);
}

static void test_cell_coordinate() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(te::assoc_grid_coord(0.0, 0.5) == 0 && te::assoc_grid_coord(-0.0, 0.5) == 0 && te::assoc_grid_coord(-1e-300, 0.5) == -1);
  CHECK(te::assoc_grid_coord(0.5, 0.5) == 1 && te::assoc_grid_coord(std::nextafter(0.5, 0.0), 0.5) == 0 && te::assoc_grid_coord(-0.5, 0.5) == -1);
  CHECK(te::assoc_grid_coord(1e300, 0.5) == (1 << 30) && te::assoc_grid_coord(-1e300, 0.5) == -(1 << 30));
  CHECK(te::assoc_grid_coord(inf, 0.5) == (1 << 30) && te::assoc_grid_coord(-inf, 0.5) == -(1 << 30) && te::assoc_grid_coord(nan, 0.5) == -(1 << 30));
  CHECK(te::assoc_grid_coord(1073741824.0, 1.0) == (1 << 30) && te::assoc_grid_coord(1073741823.5, 1.0) == (1 << 30) - 1);
  // monotone
  double prev = -3e9;
  int cprev = te::assoc_grid_coord(prev, 0.37);
  for (int k = 0; k < 20000; ++k) {
    const double x = prev + uniform() * 6e5;
    const int c = te::assoc_grid_coord(x, 0.37);
    CHECK(c >= cprev);
    prev = x; cprev = c;
  }
}

// for a narrow reach2 (<= lim2), every x with fl(nu nu) <= reach2, nu = fl(x - zhat), lands within +-1 cell of zhat
static long neighbour_cases = 0;
static void neighbour(double zhat, double x, double cell) {
  const double lim2 = te::assoc_grid_narrow_limit2(cell);
  const double nu = x - zhat;
  if (!(nu * nu <= lim2)) return;           // not inside the largest narrow box: nothing is claimed
  ++neighbour_cases;
  const int d = te::assoc_grid_coord(x, cell) - te::assoc_grid_coord(zhat, cell);
  if (!(d >= -1 && d <= 1)) { std::printf("FAIL neighbour zhat %.17g x %.17g cell %.17g d %d\n", zhat, x, cell, d); ++fails; }
}
static void test_neighbour_property() {
  const double cells[] = {1e-3, 0.0078125, 0.1, 0.37, 0.45, 0.5, 1.0, 3.0, 2.5, 7.3, 1e2, 1e3};
  for (double cell : cells) {
    const double L = cell * (1.0 - 9.5367431640625e-07);
    CHECK(te::assoc_grid_narrow_limit2(cell) == L * L);
    const double reach = std::sqrt(L * L);
    // random, at every scale up to beyond the clamp, both signs
    for (int k = 0; k < 40000; ++k) {
      const double scale = std::ldexp(1.0, (int)(next_u64() % 36));            // 1 .. 2^35 cells
      const double zhat = (uniform() * 2.0 - 1.0) * scale * cell;
      const double off = (uniform() * 2.0 - 1.0) * reach * 1.0000001;
      neighbour(zhat, zhat + off, cell);
      neighbour(zhat, zhat + (off < 0 ? -reach : reach), cell);                // the farthest x the box admits, or just beyond
    }
    // adversarial: zhat and x exactly on borders and one ulp either side, at the full reach and one ulp either side of it
    const double ks[] = {0, 1, -1, 2, -2, 3, -3, 1000, -1000, 123457, -123457, 1073741822, 1073741823, 1073741824, 1073741825, 2147483648.0,
                         -1073741822, -1073741823, -1073741824, -1073741825, -2147483648.0, 3e9, -3e9};
    for (double k : ks) {
      const double border = k * cell;
      const double zs[] = {border, std::nextafter(border, -1e308), std::nextafter(border, 1e308), border + 0.5 * cell};
      for (double zhat : zs) {
        for (int s = -1; s <= 1; s += 2) {
          const double far = zhat + s * reach;
          const double xs[] = {far, std::nextafter(far, -1e308), std::nextafter(far, 1e308), zhat + s * L, zhat + s * cell * 0.999999,
                               border + s * cell, std::nextafter(border + s * cell, zhat), zhat, (k + s) * cell, (k + 2 * s) * cell};
          for (double x : xs) neighbour(zhat, x, cell);
        }
      }
    }
  }
  CHECK(neighbour_cases > 400000);
  // where the square of the limit is not a normal double no slot is narrow
  CHECK(te::assoc_grid_narrow_limit2(1e-200) == -1.0 && te::assoc_grid_narrow_limit2(1e200) == -1.0);
  const double r_ok[3] = {0.2, 0.1, 0.2}, r_wide[3] = {0.2, 0.3, 0.2}, r_nan[3] = {0.2, std::nan(""), 0.2};
  const double lim2 = te::assoc_grid_narrow_limit2(0.5);
  CHECK(te::assoc_grid_class(1.0, r_ok, lim2) == te::kAssocGridNarrow && te::assoc_grid_class(1.0, r_wide, lim2) == te::kAssocGridWide);
  CHECK(te::assoc_grid_class(1.0, r_nan, lim2) == te::kAssocGridWide && te::assoc_grid_class(std::nan(""), r_ok, lim2) == te::kAssocGridNone);
  CHECK(te::assoc_grid_class(1.0, r_ok, -1.0) == te::kAssocGridWide);
}

// the box contains the gate for well-conditioned S, and the rule never accepts what d2 <= gate rejects
static void test_box_rule() {
  long inside = 0;
  for (int k = 0; k < 20000; ++k) {
    double A[3][3], S[6], W[6];
    for (auto& r : A) for (double& v : r) v = uniform() * 2.0 - 1.0;
    int q = 0;
    for (int r = 0; r < 3; ++r)
      for (int c = r; c < 3; ++c, ++q) {
        S[q] = 0.0025 * (A[r][0] * A[c][0] + A[r][1] * A[c][1] + A[r][2] * A[c][2]) + (r == c ? 0.01 : 0.0);
      }
    if (!te::assoc_invert_s(S, W)) continue;
    const double gate = 9.0;
    const double reach2[3] = {te::assoc_grid_reach2(gate, S[0]), te::assoc_grid_reach2(gate, S[3]), te::assoc_grid_reach2(gate, S[5])};
    CHECK(reach2[0] == (gate * S[0]) * (1.0 + 1.0 / 1024.0));
    const double zhat[3] = {uniform() * 10 - 5, uniform() * 10 - 5, uniform() * 10 - 5};
    for (int t = 0; t < 8; ++t) {
      const double x = zhat[0] + (uniform() - 0.5), y = zhat[1] + (uniform() - 0.5), z = zhat[2] + (uniform() - 0.5);
      double d2;
      const bool c = te::assoc_grid_candidate(zhat, W, reach2, x, y, z, gate, &d2);
      CHECK(d2 == te::assoc_d2(zhat, W, x, y, z));
      CHECK(c == te::assoc_candidate(d2, gate));        // well-conditioned: the box loses nothing; and never more than the gate
      inside += c;
    }
  }
  CHECK(inside > 1000);
  const double zhat[3] = {0, 0, 0}, W[6] = {1, 0, 0, 1, 0, 1}, tight[3] = {1.0, 1.0, 1.0}, nanr[3] = {std::nan(""), 1.0, 1.0};
  double d2;
  CHECK(te::assoc_grid_candidate(zhat, W, tight, 1.0, 0.0, 0.0, 4.0, &d2) && d2 == 1.0);
  CHECK(!te::assoc_grid_candidate(zhat, W, tight, std::nextafter(1.0, 2.0), 0.0, 0.0, 4.0, &d2));      // inside the gate, outside the box
  CHECK(!te::assoc_grid_candidate(zhat, W, nanr, 0.5, 0.0, 0.0, 4.0, &d2));
  CHECK(!te::assoc_grid_candidate(zhat, W, tight, std::nan(""), 0.0, 0.0, 4.0, &d2));
  CHECK(!te::assoc_grid_candidate(zhat, W, tight, 1.0, 1.0, 1.0, 2.5, &d2) && d2 == 3.0);              // inside the box, outside the gate
}

// the keyed pick under any visiting order, with ties and repeats, is the first entry of the list sorted by (d2, index)
static void test_keyed_pick() {
  for (int trial = 0; trial < 2000; ++trial) {
    const int n = 1 + (int)(next_u64() % 40);
    std::vector<std::pair<double, int>> e;
    for (int i = 0; i < n; ++i) e.push_back({(double)(next_u64() % 5) * 0.25, i});     // few distinct costs: many ties
    std::vector<std::pair<double, int>> sorted = e;
    std::sort(sorted.begin(), sorted.end());
    std::vector<std::pair<double, int>> visit = e;
    for (int i = 0; i < n / 2; ++i) visit.push_back(e[next_u64() % n]);                 // repeats, as bucket collisions cause
    for (size_t i = visit.size() - 1; i > 0; --i) std::swap(visit[i], visit[next_u64() % (i + 1)]);
    te::AssocBest best = te::assoc_best_none();
    for (const auto& v : visit) te::assoc_take_keyed(best, v.first, v.second);
    CHECK(best.idx == sorted[0].second && best.d2 == sorted[0].first);
    // ... where the ascending-order rule alone (assoc_take) would depend on the order
    te::AssocBest asc = te::assoc_best_none();
    for (const auto& v : e) te::assoc_take(asc, v.first, v.second);
    CHECK(asc.idx == best.idx);
  }
  te::AssocBest none = te::assoc_best_none();
  CHECK(none.idx == -1);
  te::assoc_take_keyed(none, 0.0, 7);
  te::assoc_take_keyed(none, 0.0, 3);
  te::assoc_take_keyed(none, 0.0, 5);
  CHECK(none.idx == 3 && none.d2 == 0.0);
}

int main() {
  test_refusals();
  test_buckets();
  test_cell_coordinate();
  test_neighbour_property();
  test_box_rule();
  test_keyed_pick();
  if (fails) { std::printf("%d failure(s)\n", fails); return 1; }
  std::printf("associate grid plan host test ok (%ld neighbour cases)\n", neighbour_cases);
  return 0;
}
