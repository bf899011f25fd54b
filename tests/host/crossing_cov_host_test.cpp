// CPU only (g++ -fsanitize=address,undefined -ffp-contract=off): the HIP-free half of the crossing covariance,
// csrc/crossing_cov_plan.hpp -- the predict of a chain block against a long double evaluation of A P A^T + Q, its symmetry, the
// filler, the refusal table, and the special cases of sigma_r / sigma_t / ok.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../target_estimation_amd/csrc/crossing_cov_plan.hpp"

using namespace te;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// THE BOUND.  crossing_predict_block forms every entry as a sum of terms a_i P(i, j) a_j (+ Q) with a in {1, dt, hdt}.  A term
// passes through at most 7 roundings of precision T: hdt itself (0.5 dt is exact, the product with dt rounds once) on either side
// (2), two fma in the row stage (2), two in the column stage (2), and the addition of Q (1).  With u the unit round-off every term
// is therefore off by at most a factor (1 + u)^7, i.e. relatively gamma_7 = 7u / (1 - 7u) (Higham, Accuracy and Stability, Lemma
// 3.1), so  |computed - exact| <= gamma_7 (|A| |P| |A|^T + |Q|)  entry by entry.  The long double reference carries the same
// seven roundings at 2^-64: added as 7 * LDBL_EPSILON of the same magnitude.
template <typename T> static long double unit_roundoff() { return (long double)std::numeric_limits<T>::epsilon() / 2; }

template <int NB, typename T>
static void reference(const T (&P)[NB][NB], const T (&Q)[NB][NB], T dt, long double (&out)[NB][NB], long double (&mag)[NB][NB]) {
  long double A[NB][NB] = {};
  for (int i = 0; i < NB; ++i) {
    A[i][i] = 1.0L;
    if (i + 1 < NB) A[i][i + 1] = (long double)dt;
    if (i + 2 < NB) A[i][i + 2] = 0.5L * (long double)dt * (long double)dt;
  }
  for (int b = 0; b < NB; ++b)
    for (int c = 0; c < NB; ++c) {
      long double v = 0, m = 0;
      for (int i = 0; i < NB; ++i)
        for (int j = 0; j < NB; ++j) {
          const long double t = A[b][i] * (long double)P[i][j] * A[c][j];
          v += t;
          m += fabsl(t);
        }
      out[b][c] = v + (long double)Q[b][c];
      mag[b][c] = m + fabsl((long double)Q[b][c]);
    }
}

template <int NB, typename T>
static void test_predict(const char* name) {
  std::mt19937_64 rng(20260 + NB + sizeof(T));
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  const long double u = unit_roundoff<T>();
  const long double gamma7 = 7 * u / (1 - 7 * u);
  long double worst = 0;
  const double dts[] = {0.0, 0.004, 0.25, 1.0, 3.75, 60.0, -0.5};
  for (double dtd : dts)
    for (int trial = 0; trial < 200; ++trial) {
      const bool symmetric = trial % 2 == 0;
      const double scale = std::pow(10.0, (double)(trial % 7) - 3.0);
      T P[NB][NB], Q[NB][NB], P0[NB][NB];
      for (int i = 0; i < NB; ++i)
        for (int j = 0; j < NB; ++j) { P[i][j] = (T)(scale * uni(rng)); Q[i][j] = (T)(1e-3 * scale * uni(rng)); }
      if (symmetric)
        for (int i = 0; i < NB; ++i)
          for (int j = 0; j < i; ++j) { P[i][j] = P[j][i]; Q[i][j] = Q[j][i]; }
      for (int i = 0; i < NB; ++i)
        for (int j = 0; j < NB; ++j) P0[i][j] = P[i][j];
      const T dt = (T)dtd;
      long double ref[NB][NB], mag[NB][NB];
      reference<NB, T>(P0, Q, dt, ref, mag);
      crossing_predict_block<NB, T>(P, Q, dt);
      for (int b = 0; b < NB; ++b)
        for (int c = 0; c < NB; ++c) {
          const long double bound = gamma7 * mag[b][c] + 7 * (long double)LDBL_EPSILON * mag[b][c];
          const long double err = fabsl((long double)P[b][c] - ref[b][c]);
          if (mag[b][c] > 0 && err / mag[b][c] > worst) worst = err / mag[b][c];
          CHECK(err <= bound);
          // SYMMETRY.  A symmetric block with a symmetric Q comes back symmetric: bit for bit in every pair whose two entries are
          // the same expression -- all of NB = 2, and (0, 2), (1, 2) of NB = 3 -- and within the two entries' bounds for (0, 1) of
          // NB = 3, whose row-stage and column-stage sums associate differently.  (The kernel reads only entry (0, 0) of a block and
          // reports the upper triangle of Sigma, so its output is symmetric by construction.)
          if (symmetric && c > b) {
            if (NB == 2 || c == 2) CHECK(P[b][c] == P[c][b]);
            else CHECK(fabsl((long double)P[b][c] - (long double)P[c][b]) <= 2 * bound);
          }
        }
    }
  std::printf("predict NB=%d %s: worst error / magnitude %.3Lg (gamma_7 = %.3Lg)\n", NB, name, worst, gamma7);
}

static void test_filler() {
  const CrossingCovRow f = crossing_cov_filler();
  for (int c = 0; c < 6; ++c) CHECK(f.cov[c] == 0.0 && !std::signbit(f.cov[c]));
  CHECK(f.sigma[0] == -1.0 && f.sigma[1] == -1.0 && f.ok == 0);
  std::vector<double> cov(18, 7.0), sigma(6, 7.0);
  std::vector<unsigned char> ok(3, 9);
  crossing_cov_fill(1, cov.data(), sigma.data(), ok.data());
  for (int i = 0; i < 18; ++i) CHECK(cov[(size_t)i] == ((i >= 6 && i < 12) ? 0.0 : 7.0));
  for (int i = 0; i < 6; ++i) CHECK(sigma[(size_t)i] == ((i == 2 || i == 3) ? -1.0 : 7.0));
  CHECK(ok[0] == 9 && ok[1] == 0 && ok[2] == 9);
  crossing_cov_fill(2, cov.data(), nullptr, nullptr);   // the optional outputs may be absent
  for (int i = 12; i < 18; ++i) CHECK(cov[(size_t)i] == 0.0);
  CHECK(sigma[4] == 7.0 && ok[2] == 9);
}

static bool refused(bool delta, bool origin, double radius, bool cov, bool sigma, bool ok, double sr, double st, bool rows, long n, long size) {
  try { check_crossing_cov_args(delta, origin, radius, cov, sigma, ok, sr, st, rows, n, size); } catch (const std::invalid_argument&) { return true; }
  return false;
}

static void test_refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  struct Case { bool delta, origin; double radius; bool cov, sigma, ok; double sr, st; bool rows; long n, size; bool refuse; };
  const Case table[] = {
      {true, true, 1.0, true, true, true, inf, inf, false, 130, 130, false},     // the full dense call
      {true, false, 0.0, true, false, false, inf, inf, false, 130, 130, false},  // covariance only: no origin, the radius is not read
      {true, false, nan, true, false, false, inf, inf, false, 0, 130, false},
      {true, true, 1.0, true, true, false, 0.5, 0.002, true, 8192, 5, false},    // a list is not bounded by the batch's size
      {true, true, 1.0, true, false, true, 0.0, 0.0, true, 1, 0, false},         // zero thresholds are thresholds
      {false, true, 1.0, true, true, true, inf, inf, false, 1, 1, true},         // a NULL delta
      {true, true, 1.0, false, true, true, inf, inf, false, 1, 1, true},         // a NULL cov_out
      {true, false, 1.0, true, true, false, inf, inf, false, 1, 1, true},        // sigma without origin
      {true, false, 1.0, true, false, true, inf, inf, false, 1, 1, true},        // ok without origin
      {true, true, 0.0, true, true, true, inf, inf, false, 1, 1, true},          // radius 0 with origin
      {true, true, -1.0, true, false, false, inf, inf, false, 1, 1, true},       // radius < 0 with origin
      {true, true, nan, true, true, true, inf, inf, false, 1, 1, true},          // radius NaN with origin
      {true, true, 1.0, true, true, true, nan, inf, false, 1, 1, true},          // NaN thresholds
      {true, true, 1.0, true, true, true, inf, nan, false, 1, 1, true},
      {true, false, 0.0, true, false, false, nan, inf, false, 1, 1, true},       // ... whether or not they are used
      {true, true, 1.0, true, true, true, inf, inf, false, -1, 1, true},         // n out of range
      {true, true, 1.0, true, true, true, inf, inf, false, 131, 130, true},
      {true, true, 1.0, true, true, true, inf, inf, true, 8193, 100000, true},
      {true, true, 1.0, true, true, true, inf, inf, true, -1, 100000, true},
  };
  for (const Case& c : table) {
    const bool r = refused(c.delta, c.origin, c.radius, c.cov, c.sigma, c.ok, c.sr, c.st, c.rows, c.n, c.size);
    if (r != c.refuse) std::printf("refusal table: row %ld\n", (long)(&c - table));
    CHECK(r == c.refuse);
  }
  bool threw = false;
  try { check_crossing_cov_one_shard(2); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw);
  check_crossing_cov_one_shard(1);
  CHECK(kCrossingCovMaxRows == 8192);
}

static void test_sigma() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const double o[3] = {0.0, 0.0, 0.0};
  double sr, st;
  // along x at distance 2, closing at 4 m/s: sigma_r = sqrt(Sxx), sigma_t = sigma_r / 4
  const double S[6] = {0.25, 0.01, 0.02, 9.0, 0.03, 16.0};
  const double p[3] = {2.0, 0.0, 0.0}, v[3] = {-4.0, 1.0, 7.0};
  crossing_sigma(S, p, v, o, sr, st);
  CHECK(sr == 0.5 && st == 0.125);
  // a general direction against the form written out in long double
  const double p2[3] = {1.0, -2.0, 2.0}, v2[3] = {0.5, 0.25, -3.0}, o2[3] = {0.5, 0.5, -0.5};
  crossing_sigma(S, p2, v2, o2, sr, st);
  {
    const long double d[3] = {0.5L, -2.5L, 2.5L};
    const long double len = sqrtl(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const long double n[3] = {d[0] / len, d[1] / len, d[2] / len};
    const long double M[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
    long double form = 0, nv = 0;
    for (int i = 0; i < 3; ++i) { nv += n[i] * v2[i]; for (int j = 0; j < 3; ++j) form += n[i] * M[i][j] * n[j]; }
    CHECK(fabsl(sr - sqrtl(form)) <= 1e-14L * sqrtl(form));
    CHECK(fabsl(st - sqrtl(form) / fabsl(nv)) <= 1e-14L * sqrtl(form) / fabsl(nv));
  }
  // zero radial speed: +inf (tangential motion never closes)
  const double vt[3] = {0.0, 3.0, -1.0};
  crossing_sigma(S, p, vt, o, sr, st);
  CHECK(sr == 0.5 && st == inf);
  // a negative form is not clamped: NaN
  const double Sneg[6] = {-0.25, 0, 0, 1, 0, 1};
  crossing_sigma(Sneg, p, v, o, sr, st);
  CHECK(sr != sr && st != st);
  // the crossing at the origin itself: NaN
  crossing_sigma(S, o, v, o, sr, st);
  CHECK(sr != sr);
  // the candidate rule and the ok rule: <=, a NaN on either side rejects, +inf switches a bound off
  CHECK(crossing_candidate(0.0) && crossing_candidate(-0.0) && crossing_candidate(inf) && !crossing_candidate(-1.0) && !crossing_candidate(nan));
  CHECK(crossing_ok(1.0, 0.5, 0.002, 0.5, 0.002));
  CHECK(!crossing_ok(1.0, 0.5, 0.0020000001, 0.5, 0.002) && !crossing_ok(1.0, 0.50001, 0.002, 0.5, 0.002));
  CHECK(crossing_ok(1.0, 0.5, inf, 0.5, inf) && !crossing_ok(1.0, 0.5, inf, 0.5, 1e300));
  CHECK(!crossing_ok(1.0, nan, 0.0, inf, inf) && !crossing_ok(1.0, 0.0, nan, inf, inf));
  CHECK(!crossing_ok(-1.0, 0.0, 0.0, inf, inf) && !crossing_ok(nan, 0.0, 0.0, inf, inf));
  CHECK(crossing_ok(0.0, 0.0, 0.0, 0.0, 0.0));
}

int main() {
  test_predict<2, double>("double");
  test_predict<3, double>("double");
  test_predict<2, float>("float");
  test_predict<3, float>("float");
  test_filler();
  test_refusals();
  test_sigma();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("crossing cov host test ok\n");
  return 0;
}
