// crossing_cov.hip -- crossing_cov_kernel: the position covariance of a target at its sphere crossing, and the spreads sigma_r /
// sigma_t that follow from it (crossing_cov.hpp).  A unit of its own: no step kernel is touched.
#include "crossing_cov.hpp"

#include "kf_aux.hpp"

namespace te {

// A thread per row.  The row's delta is read first: a row that is no candidate (delta negative or NaN, slot -1 or outside the
// batch) writes the filler and loads no record word.  A candidate loads x, the stored P words of the position chains {r, r + K,
// (r + 2K)}, r = 0..2 -- through the layout's accessors, a flagged uniform tile's words from the tile's block, as get_state_kernel
// and innov_kernel do -- the chains' Q words of the slot's class, and t_base[slot] for an absolute t1.
// Sigma(r, c) = (A B A^T + Qb)[0][0] with B(i, j) = P(r + iK, c + jK), Qb(i, j) = Q(r + iK, c + jK): one call of
// crossing_predict_block per stored pair r <= c, in the batch's precision.  The separable layouts store no word between two axes:
// those entries are exact zeros and cost nothing.  Only rows 0..2 of A(tau) enter, which are [1 tau (tau^2/2)] in every model:
// the EKF's Jacobian is never formed.  Plain loads and stores, no LDS, no atomics.
template <class M, typename T, int G, int LAYOUT>
__global__ __launch_bounds__(64) void crossing_cov_kernel(const CrossingCovArgs a) {
#pragma clang fp contract(off)
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N, K = C::K, NB = C::NB;
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  if (a.batch != nullptr && a.batch[row] != a.batch_index) return;   // another batch's launch (or the orphans') writes this row
  const double delta = a.delta[row];
  long slot = -1;
  if (crossing_candidate(delta)) slot = a.slots ? (long)a.slots[row] : row;
  if (slot < 0 || slot >= a.size) {
    crossing_cov_fill(row, a.cov, a.sigma, a.ok);
    return;
  }
  const bool own = a.t1 != a.t1;
  const double dq = own ? 0.0 : te_clock_offset(a.t1, a.t_base[slot], a.t_acc);
  const T tau = own ? (T)delta : (T)(delta + dq);   // the offset the query's pose was taken at (sphere_query_values)
  const T* qr = static_cast<const T*>(a.qr) + (a.cls ? (long)a.cls[slot] * C::QR_WORDS : 0L);
  bool uni = false;
  if constexpr (C::UT) uni = a.tile_uni != nullptr && a.tile_uni[slot / C::TPW] != 0;
  auto Pget = [&](int r, int c) -> T {
    if constexpr (C::UT) {
      const int w = C::PWORD.v[r][c];
      if (uni && w >= 0 && C::LIN.idx[w] >= 0) return (T)a.tile_blk[(slot / C::TPW) * C::LW + C::LIN.idx[w]];
    }
    return state_get<C, T>(a.rec, slot, r, c);
  };
  double S[6];
#pragma unroll
  for (int r = 0, k = 0; r < 3; ++r) {
#pragma unroll
    for (int c = r; c < 3; ++c, ++k) {
      if (C::SEP && r != c) { S[k] = 0.0; continue; }
      T B[NB][NB], Qb[NB][NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          B[i][j] = Pget(r + i * K, c + j * K);
          const int qw = C::QWORD.v[r + i * K][c + j * K];
          Qb[i][j] = qw >= 0 ? qr[qw] : (T)0;
        }
      }
      crossing_predict_block<NB, T>(B, Qb, tau);
      S[k] = (double)B[0][0];
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) a.cov[row * 6 + k] = S[k];
  if (!a.have_origin) return;
  T x[N];
#pragma unroll
  for (int r = 0; r < N; ++r) x[r] = state_get<C, T>(a.rec, slot, r, N);
  T pose7[7], twist6[6], acc6[6];
  derive_outputs<M, T>(x, true, tau, pose7, twist6, acc6);
  const double p[3] = {(double)pose7[0], (double)pose7[1], (double)pose7[2]};
  const double v[3] = {(double)twist6[0], (double)twist6[1], (double)twist6[2]};
  double sr, st;
  crossing_sigma(S, p, v, a.origin, sr, st);
  if (a.sigma) { a.sigma[row * 2] = sr; a.sigma[row * 2 + 1] = st; }
  if (a.ok) a.ok[row] = crossing_ok(delta, sr, st, a.sigma_r_max, a.sigma_t_max) ? 1 : 0;
}

__global__ void crossing_cov_orphans_kernel(const int* batch, long n, int n_batches, double* cov, double* sigma, unsigned char* ok) {
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int b = batch[row];
  if (b < 0 || b >= n_batches) crossing_cov_fill(row, cov, sigma, ok);
}

void launch_crossing_cov_orphans(const int* batch, long n, int n_batches, double* cov, double* sigma, unsigned char* ok, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(crossing_cov_orphans_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, batch, n, n_batches, cov, sigma, ok);
}

namespace {

template <class M, typename T, int G, int LAYOUT>
void launch(const CrossingCovArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL((crossing_cov_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
}

// every lanes-per-target count a model's layouts come in (te_layout.hpp: G divides K)
template <class M, typename T>
CrossingCovLaunch pick(int g, int layout, bool shared_axes) {
  if (shared_axes) {
    if constexpr (sizeof(T) == 8) return &launch<M, T, 1, LAYOUT_SEPARABLE_SHARED>;
    return nullptr;
  }
  if (layout == LAYOUT_SEPARABLE) return g == 1 ? &launch<M, T, 1, LAYOUT_SEPARABLE> : nullptr;
  if (layout == LAYOUT_SEPARABLE_PACKED) return g == 1 ? &launch<M, T, 1, LAYOUT_SEPARABLE_PACKED> : nullptr;
  if (layout == LAYOUT_FULL) {
    if (g == 1) return &launch<M, T, 1, LAYOUT_FULL>;
    if (g == 3) return &launch<M, T, 3, LAYOUT_FULL>;
    if constexpr (M::K == 6) {
      if (g == 2) return &launch<M, T, 2, LAYOUT_FULL>;
      if (g == 6) return &launch<M, T, 6, LAYOUT_FULL>;
    }
    return nullptr;
  }
  if (layout == LAYOUT_PACKED) {
    if (g == 1) return &launch<M, T, 1, LAYOUT_PACKED>;
    if (g == 3) return &launch<M, T, 3, LAYOUT_PACKED>;
    if constexpr (M::K == 6) {
      if (g == 2) return &launch<M, T, 2, LAYOUT_PACKED>;
      if (g == 6) return &launch<M, T, 6, LAYOUT_PACKED>;
    }
    return nullptr;
  }
  return nullptr;
}

template <class M>
CrossingCovLaunch pick_dtype(int dtype, int g, int layout, bool shared_axes) {
  if (dtype == F64) return pick<M, double>(g, layout, shared_axes);
  if (dtype == F32) return pick<M, float>(g, layout, shared_axes);
  return nullptr;
}

}  // namespace

CrossingCovLaunch crossing_cov_launcher(int type, int dtype, int g, int layout, bool shared_axes) {
  switch (type) {
    case UNIFORM_VELOCITY: return pick_dtype<ModelUV>(dtype, g, layout, shared_axes);
    case UNIFORM_ACCELERATION: return pick_dtype<ModelUA>(dtype, g, layout, shared_axes);
    case ANGULAR_RATES: return pick_dtype<ModelAR>(dtype, g, layout, shared_axes);
    case ANGULAR_VELOCITIES: return pick_dtype<ModelAV>(dtype, g, layout, shared_axes);
  }
  return nullptr;
}

}  // namespace te
