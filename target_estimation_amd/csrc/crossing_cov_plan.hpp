// crossing_cov_plan.hpp -- no HIP: everything about "position covariance and time spread at a sphere crossing" (target_batch_c.h,
// target_batch_crossing_cov_dev) that is not a kernel -- the predict of one position chain block, the sphere outputs sigma_r /
// sigma_t and the ok rule, the filler row and the argument checks.  crossing_cov.hip (the kernel), Batch / Shard / TargetManager
// (the host side) and tests/host/crossing_cov_host_test.cpp (g++ alone) all build this header.
#pragma once
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

#if defined(__HIPCC__)
#define TE_CCOV_HD __host__ __device__
#else
#define TE_CCOV_HD
#endif

namespace te {

constexpr long kCrossingCovMaxRows = 8192;   // TARGET_CROSSING_COV_MAX_ROWS: the entries of a slot list

// the one fused operation of the predict, in both precisions (the builtins are the compiler's own in host and device code)
TE_CCOV_HD inline double ccov_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
TE_CCOV_HD inline float ccov_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// THE PREDICT of one NB x NB block of the covariance of [p v (a)] chains over the horizon dt: P <- A P A^T + Q with
// A = [1 dt (dt^2/2); 0 1 (dt); (0 0 1)].  P(i, j) is the covariance of state i of one chain with state j of another (the same
// chain in the separable layouts: the block is then the chain's own, and symmetric).  Statement for statement the predict of
// sep_linear_cov / sep_gate_predict_P (kf_step_sep.hpp): rows, then columns, then + Q, explicit fma only, contraction off.
// Entry [0][0] of the result is the position-position entry Sigma(r, c) of the two chains' axes.
template <int NB, typename T>
TE_CCOV_HD inline void crossing_predict_block(T (&P)[NB][NB], const T (&Q)[NB][NB], T dt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const T hdt = (T)0.5 * dt * dt;
  // AP = A P (rows)
  for (int b = 0; b + 1 < NB; ++b) {
    for (int c = 0; c < NB; ++c) {
      T v = ccov_fma(dt, P[b + 1][c], P[b][c]);
      if (NB == 3 && b == 0) v = ccov_fma(hdt, P[b + 2][c], v);
      P[b][c] = v;
    }
  }
  // (AP) A^T (columns), + Q
  for (int b = 0; b < NB; ++b)
    for (int c = 0; c < NB; ++c) {
      T v = P[b][c];
      if (c + 1 < NB) {
        v = ccov_fma(dt, P[b][c + 1], v);
        if (NB == 3 && c == 0) v = ccov_fma(hdt, P[b][c + 2], v);
      }
      P[b][c] = v + Q[b][c];
    }
}

// THE SPHERE OUTPUTS, all in double.  S: the upper triangle of Sigma (xx xy xz yy yz zz); p, v: position and linear velocity at the
// crossing; o: the sphere's origin.  n = (p - o) / |p - o|; sigma_r = sqrt(n^T Sigma n); sigma_t = sigma_r / |n . v|, +inf when
// n . v == 0.  Nothing is clamped: a negative form or |p - o| == 0 gives NaN.
TE_CCOV_HD inline void crossing_sigma(const double* S, const double* p, const double* v, const double* o, double& sigma_r, double& sigma_t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
  const double len = sqrt(dx * dx + dy * dy + dz * dz);
  const double nx = dx / len, ny = dy / len, nz = dz / len;
  const double sx = S[0] * nx + S[1] * ny + S[2] * nz;
  const double sy = S[1] * nx + S[3] * ny + S[4] * nz;
  const double sz = S[2] * nx + S[4] * ny + S[5] * nz;
  const double form = nx * sx + ny * sy + nz * sz;
  const double nv = nx * v[0] + ny * v[1] + nz * v[2];
  sigma_r = sqrt(form);
  sigma_t = nv == 0.0 ? (double)INFINITY : sigma_r / fabs(nv);
}
// THE CANDIDATE RULE: a row whose delta is negative or NaN is none (-1 is the library's "no intersection")
TE_CCOV_HD inline bool crossing_candidate(double delta) { return delta >= 0.0; }
// THE OK RULE: the comparisons are <=, so a NaN spread rejects; either bound may be +inf
TE_CCOV_HD inline bool crossing_ok(double delta, double sigma_r, double sigma_t, double sigma_r_max, double sigma_t_max) {
  return delta >= 0.0 && sigma_r <= sigma_r_max && sigma_t <= sigma_t_max;
}

// One row of a result.  The default is THE FILLER: what a non-candidate, a slot of -1 and an unknown id get.
struct CrossingCovRow {
  double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double sigma[2] = {-1.0, -1.0};
  unsigned char ok = 0;
};
inline CrossingCovRow crossing_cov_filler() { return CrossingCovRow{}; }
TE_CCOV_HD inline void crossing_cov_fill(long row, double* cov, double* sigma, unsigned char* ok) {
  for (int c = 0; c < 6; ++c) cov[row * 6 + c] = 0.0;
  if (sigma) { sigma[row * 2] = -1.0; sigma[row * 2 + 1] = -1.0; }
  if (ok) ok[row] = 0;
}

// THE REFUSALS.  have_*: whether the pointer was given; rows: the call carries a slot list (n <= kCrossingCovMaxRows), else it is
// dense over a batch of `size` targets (n <= size).  Throws std::invalid_argument; the caller has enqueued nothing yet.
inline void check_crossing_cov_args(bool have_delta, bool have_origin, double radius, bool have_cov, bool have_sigma, bool have_ok,
                                    double sigma_r_max, double sigma_t_max, bool rows, long n, long size) {
  const std::string pre = "target_estimation_amd: crossing_cov: ";
  if (!have_delta) throw std::invalid_argument(pre + "delta is required");
  if (!have_cov) throw std::invalid_argument(pre + "cov_out is required");
  if (have_sigma && !have_origin) throw std::invalid_argument(pre + "sigma_out without origin: there is no sphere to measure against");
  if (have_ok && !have_origin) throw std::invalid_argument(pre + "ok_out without origin: there is no sphere to measure against");
  if (have_origin && !(radius > 0.0)) throw std::invalid_argument(pre + "radius must be > 0 with an origin, got " + std::to_string(radius));
  if (sigma_r_max != sigma_r_max || sigma_t_max != sigma_t_max) throw std::invalid_argument(pre + "a threshold is NaN (+inf switches one off)");
  if (n < 0) throw std::invalid_argument(pre + "n must be >= 0, got " + std::to_string(n));
  if (rows && n > kCrossingCovMaxRows)
    throw std::invalid_argument(pre + "a slot list holds at most " + std::to_string(kCrossingCovMaxRows) + " entries, got " + std::to_string(n));
  if (!rows && n > size) throw std::invalid_argument(pre + "the dense form serves rows 0..size-1: n " + std::to_string(n) + " > size " + std::to_string(size));
}
// ... and of the manager's device form, which leaves its result on ONE device
inline void check_crossing_cov_one_shard(long shards) {
  if (shards > 1)
    throw std::runtime_error("target_estimation_amd: crossing_cov_dev: the manager spans " + std::to_string(shards) +
                             " shards, so there is no single device to read the rows from (use crossing_cov_batch, which goes by id)");
}

}  // namespace te
