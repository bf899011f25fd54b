// CPU-only test of csrc/track_merge_plan.hpp, the HIP-free half of the duplicate-track search: the refusal table; the claim that a
// pair's reach2 never exceeds the larger of its two rows' reach2 (random Sigma and adversarial ones: equal, one ulp apart, 2^60
// apart, subnormal); the neighbour property for narrow pairs (random, on cell borders, one ulp either side, negative coordinates,
// at the clamp); d2 symmetry under the (lo, hi) order; merge_pair_candidate on coupled, well- and ill-conditioned pair sums against
// a long double Cholesky solve (a derived forward bound on d2, the decision away from the gate and the box edges, lo and hi
// swapped); the keyed pick under shuffled visiting orders with repeats; the classes and the survivor rule.  g++ alone, sanitised,
// contraction off.
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

// ---- merge_pair_candidate on COUPLED pair sums against a long double Cholesky solve -------------------------------------------
// Sigma = s U diag(r^2, 1, r^-2) U^T in a random frame U (cond = r^4, r up to 30), the partner's Sigma the same under a congruence
// close to the identity or drawn afresh; nu = G u sqrt(v), G the factor of C, so that d2 = v is planted on both sides of the gate.
//
// THE BOUND.  Write F = ||C||_F, det = det C, u = 2^-53, gamma_k = k u / (1 - k u), l1 >= l2 >= l3 the eigenvalues of C; every
// |C_ij| <= F, l1 <= F, ||nu||^2 <= l1 d2 <= F d2, and 1 / l3 = l1 l2 / det <= F^2 / det.  merge_pair_candidate forms
//   (i)   C = fl(Sigma_lo + Sigma_hi) word by word: ||dC||_F <= u F, so d2 moves by at most ||C^-1|| ||dC|| d2 <= u (F^3 / det) d2;
//   (ii)  nu = fl(z_hi - z_lo): |dnu_a| <= u |nu_a|, d2 moves by 2 |nu^T C^-1 dnu| <= 2 u sqrt(l1 / l3) d2 <= 2 u (F^3 / det) d2;
//   (iii) six cofactors fl(fl(a b) - fl(c d)): each off by at most gamma_2 (|a b| + |c d|) <= gamma_2 F^2; as a matrix E,
//         |nu^T E nu| <= ||E||_F ||nu||^2 <= 3 gamma_2 F^2 ||nu||^2, which over det is <= 3 gamma_2 (F^3 / det) d2;
//   (iv)  det = fl((S0 c00 + S1 c01) + S2 c02) from those cofactors: five roundings on every term, the terms' magnitudes at most
//         (|S0| + |S1| + |S2|) F^2 <= sqrt(3) F^3: a relative error of sqrt(3) gamma_5 F^3 / det in det, hence in d2;
//   (v)   W = fl(c / det): one rounding per word, |W_ij| <= F^2 / det: at most 3 u F^2 ||nu||^2 / det <= 3 u (F^3 / det) d2;
//   (vi)  assoc_d2: three products and two sums per t_k, three products and two sums for the form: gamma_6 on the sum of the
//         magnitudes, sum |nu_k| |W_kj| |nu_j| <= 3 F^2 ||nu||^2 / det: at most 3 gamma_6 (F^3 / det) d2.
// To first order |d2 - d2_ref| <= (1 + 2 + 6 + 5 sqrt(3) + 3 + 18) u k_adj d2_ref < 39 u k_adj d2_ref with k_adj = F^3 / det, the
// condition number of an inverse taken through the adjugate: cond(C) <= k_adj <= 3 sqrt(3) cond(C)^2, and k_adj = cond(C)^1.5
// up to that factor for the spectrum (r^2, 1, r^-2) used here.  The test allows 48 u k_adj d2_ref (the second-order terms are
// below a fifth of the first while 48 u k_adj < 0.1, which it asserts) against a reference whose own error is u_ld cond(C), 2^-11
// of that.  The decision must equal the long double one wherever d2_ref is further than that bound from the gate and every
// nu_a^2 further than 16 u (relative) from its box edge (the edge is two roundings of products, C_aa one, nu_a^2 two).
struct Chol3 { long double g[6]; bool ok; };   // lower factor, packed as the upper triangle of its transpose: xx xy xz yy yz zz
static Chol3 chol3(const long double* C) {
  Chol3 f{};
  f.ok = false;
  const long double p0 = C[0];
  if (!(p0 > 0.0L)) return f;
  f.g[0] = sqrtl(p0); f.g[1] = C[1] / f.g[0]; f.g[2] = C[2] / f.g[0];
  const long double p1 = C[3] - f.g[1] * f.g[1];
  if (!(p1 > 0.0L)) return f;
  f.g[3] = sqrtl(p1); f.g[4] = (C[4] - f.g[1] * f.g[2]) / f.g[3];
  const long double p2 = C[5] - f.g[2] * f.g[2] - f.g[4] * f.g[4];
  if (!(p2 > 0.0L)) return f;
  f.g[5] = sqrtl(p2);
  f.ok = std::isfinite((double)(p0 * p1 * p2));
  return f;
}
// nu^T C^-1 nu: G y = nu forwards, G^T w = y backwards, nu . w
static long double quad_form(const Chol3& f, const long double* nu) {
  const long double y0 = nu[0] / f.g[0];
  const long double y1 = (nu[1] - f.g[1] * y0) / f.g[3];
  const long double y2 = (nu[2] - f.g[2] * y0 - f.g[4] * y1) / f.g[5];
  const long double w2 = y2 / f.g[5];
  const long double w1 = (y1 - f.g[4] * w2) / f.g[3];
  const long double w0 = (y0 - f.g[1] * w1 - f.g[2] * w2) / f.g[0];
  return nu[0] * w0 + nu[1] * w1 + nu[2] * w2;
}

static void random_frame(double U[3][3]) {
  for (;;) {
    double a[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5}, b[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5};
    const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (na < 0.05) continue;
    for (double& v : a) v /= na;
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    for (int k = 0; k < 3; ++k) b[k] -= ab * a[k];
    const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    if (nb < 0.05) continue;
    for (double& v : b) v /= nb;
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    for (int k = 0; k < 3; ++k) { U[k][0] = a[k]; U[k][1] = b[k]; U[k][2] = c[k]; }
    return;
  }
}
// the six words of s U diag(r^2, 1, r^-2) U^T
static void coupled_sigma(double* S, double s, double r) {
  double U[3][3];
  random_frame(U);
  const double d[3] = {r * r, 1.0, 1.0 / (r * r)};
  int k = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++k) S[k] = s * (U[i][0] * d[0] * U[j][0] + U[i][1] * d[1] * U[j][1] + U[i][2] * d[2] * U[j][2]);
}
// M S M^T for M = I + e N, N random: the predecessor's Sigma, slightly perturbed
static void perturbed(const double* S, double e, double* out) {
  const double full[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
  double M[3][3], T[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[i][j] = (i == j ? 1.0 : 0.0) + e * (uniform() - 0.5);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { T[i][j] = 0.0; for (int k = 0; k < 3; ++k) T[i][j] += M[i][k] * full[k][j]; }
  int w = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++w) { out[w] = 0.0; for (int k = 0; k < 3; ++k) out[w] += T[i][k] * M[j][k]; }
}

static void test_coupled_pairs_against_long_double() {
  const double u = std::ldexp(1.0, -53), gate = 9.0;
  const double ratios[] = {1.0, 3.0, 10.0, 30.0};
  int cases = 0, decided = 0, ill = 0, correlated = 0, candidates = 0, rejected_by_gate = 0, rejected_by_box = 0;
  double worst_share = 0.0, worst_rel = 0.0;
  for (int t = 0; t < 800; ++t) {
    const double r = ratios[t % 4];
    double all[20] = {};
    double* lo = all;
    double* hi = all + 10;
    coupled_sigma(lo + 3, 0.0025 * (0.5 + uniform()), r);
    if (t % 8 < 6) perturbed(lo + 3, 1e-3, hi + 3); else coupled_sigma(hi + 3, 0.0025 * (0.5 + uniform()), ratios[(t / 8) % 4]);
    long double C[6];
    for (int k = 0; k < 6; ++k) C[k] = (long double)lo[3 + k] + (long double)hi[3 + k];
    const Chol3 f = chol3(C);
    CHECK(f.ok);
    if (!f.ok) continue;
    // nu = G dir sqrt(v): d2 = v up to the rounding of the positions
    double dir[3] = {uniform() - 0.5, uniform() - 0.5, uniform() - 0.5};
    const double nd = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-30;
    const double v = t % 5 == 4 ? gate * (1.0 + 2.0 * uniform()) : gate * uniform();
    const double sv = std::sqrt(v) / nd;
    const long double off[3] = {f.g[0] * dir[0] * sv, (f.g[1] * dir[0] + f.g[3] * dir[1]) * sv, (f.g[2] * dir[0] + f.g[4] * dir[1] + f.g[5] * dir[2]) * sv};
    for (int a = 0; a < 3; ++a) { lo[a] = (uniform() - 0.5) * 16.0; hi[a] = lo[a] + (double)off[a]; }
    long double nu[3];
    for (int a = 0; a < 3; ++a) nu[a] = (long double)hi[a] - (long double)lo[a];
    const long double ref = quad_form(f, nu);
    long double F2 = 0.0L;
    for (int k = 0; k < 6; ++k) F2 += (k == 0 || k == 3 || k == 5 ? 1.0L : 2.0L) * C[k] * C[k];
    const long double F = sqrtl(F2), piv = f.g[0] * f.g[3] * f.g[5], det = piv * piv;
    const double k_adj = (double)(F * F * F / det);
    CHECK(48.0 * u * k_adj < 0.1);
    const double bound = 48.0 * u * k_adj * (double)ref;
    double d2 = 0.0;
    const bool cand = te::merge_pair_candidate(lo, hi, gate, &d2);
    const double err = std::fabs((double)((long double)d2 - ref));
    CHECK(d2 >= 0.0 && err <= bound);
    ++cases;
    if (bound > 0.0) worst_share = std::max(worst_share, err / bound);
    worst_rel = std::max(worst_rel, err / std::max((double)ref, 1.0));
    if (k_adj >= 1e5) ++ill;
    static const int diag[3] = {0, 3, 5}, off_word[3][3] = {{1, 0, 3}, {2, 0, 5}, {4, 3, 5}};   // xy, xz, yz and their two diagonal words
    for (const int* w : off_word)
      if (std::fabs((double)C[w[0]]) >= 0.3 * std::sqrt((double)(C[w[1]] * C[w[2]]))) { ++correlated; break; }
    // the decision, away from the gate and the box edges
    bool in_box = true, box_clear = true;
    for (int a = 0; a < 3; ++a) {
      const long double edge = (long double)gate * C[diag[a]] * (1.0L + 0x1p-10L), n2 = nu[a] * nu[a];
      in_box = in_box && n2 <= edge;
      box_clear = box_clear && fabsl(n2 - edge) > 16.0L * u * edge;
    }
    const bool gate_clear = std::fabs((double)(ref - (long double)gate)) > bound;
    if (gate_clear && box_clear) {
      ++decided;
      const bool want = ref <= (long double)gate && in_box;
      CHECK(cand == want);
      candidates += want;
      rejected_by_gate += in_box && !(ref <= (long double)gate);
      rejected_by_box += !in_box && ref <= (long double)gate;
    }
    // swapping lo and hi cannot change a bit: through the walk's (self, other) form, and with the rows handed over the other way
    double d_ab = 0.0, d_ba = 0.0, d_sw = 0.0;
    const bool ok_ab = te::merge_pair_candidate_of(all, 0, 1, gate, &d_ab), ok_ba = te::merge_pair_candidate_of(all, 1, 0, gate, &d_ba);
    const bool ok_sw = te::merge_pair_candidate(hi, lo, gate, &d_sw);
    CHECK(ok_ab == cand && ok_ba == cand && ok_sw == cand);
    CHECK(std::memcmp(&d_ab, &d2, sizeof d2) == 0 && std::memcmp(&d_ba, &d2, sizeof d2) == 0 && std::memcmp(&d_sw, &d2, sizeof d2) == 0);
  }
  std::printf("coupled pairs: %d cases, %d ill-conditioned (k_adj >= 1e5), %d correlated, %d decided (%d candidates, %d rejected by the gate, %d by the box alone);"
              " worst d2 error %.3e of max(d2, 1), %.3f of the bound\n", cases, ill, correlated, decided, candidates, rejected_by_gate, rejected_by_box,
              worst_rel, worst_share);
  CHECK(cases >= 790 && ill >= 200 && correlated >= 400 && decided >= 780 && candidates >= 300 && rejected_by_gate >= 50);
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
  test_coupled_pairs_against_long_double();
  test_classes_and_survivor();
  test_keyed_pick();
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("track merge plan host test ok\n");
  return 0;
}
