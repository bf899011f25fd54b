// kf_reacquire_impl.hpp -- included by kf_reacquire_{uv,ua,ar,av}.hip: the launch behind a gated tick that keeps every slot's
// rejection run and re-initialises a target from the tick's measurement on its K-th consecutive rejection (target_batch_c.h,
// target_reacquire_c).  One motion model per translation unit, one instance per (precision, lanes, layout) that
// init_kernel has.  OpsImpl::reacquire (kf_ops_impl.hpp) launches it through launch_reacquire.
#pragma once
#include "kf_ops.hpp"

namespace te {

constexpr int kReacquireBlock = 256;   // four wavefronts of 64 consecutive slots

// Thread per slot.  STREAMING part, every lane: the NIS the tick's step has just written, the caller's mask byte and the run c;
//   no measurement                      c unchanged                  event 0
//   accepted (nis <= gate, as the step) c = 0                        event 0
//   rejected                            c' = min(c + 1, 127), c = c' event c'
//   rejected and re-initialised         c = 0                        event 0x80 | c'
// A wavefront without a lane that has k > 0 and c' >= k leaves here: about 11 B per target, no record touched.  RARE part: such a
// lane forms x0 from the tick's measurement as init_kernel does (v0 = a0 = 0) and re-initialises iff every component is finite;
// its record then is, bit for bit, init_kernel's with P0 = p0_tab[p0_idx[slot]] and unwrap memory 0.  The clock and the
// measurement counter of the slot are not touched.
// Uniform tiles (Cfg::UT): a wavefront is one tile.  Ahead of any re-initialisation a flagged tile is settled as
// settle_tiles_kernel does -- every lane copies the tile's block into its own record -- and one lane clears the flag.
template <class M, typename T, int G, int LAYOUT>
__global__ __launch_bounds__(kReacquireBlock) void reacquire_kernel(const ReacquireArgs a) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  const long e = (long)blockIdx.x * kReacquireBlock + threadIdx.x;
  const bool valid = e < a.n;
  unsigned c1 = 0;
  unsigned char ev = 0, run = 0;
  bool store_run = false, cand = false;
  if (valid && (a.has_meas == nullptr || a.has_meas[e] != 0)) {
    const unsigned c = a.run[e];
    const double nis = a.nis[e];
    store_run = true;
    if (!(nis <= a.gate)) {   // rejected (a NaN rejects), as the step decided
      c1 = c + 1 < 127u ? c + 1 : 127u;
      ev = (unsigned char)c1; run = (unsigned char)c1;
      cand = a.k > 0 && c1 >= (unsigned)a.k;
    }
  }
  if (__ballot(cand) == 0ull) {   // the common case
    if (store_run) a.run[e] = run;
    if (valid && a.event != nullptr) a.event[e] = ev;
    return;
  }
  T x0[N];
#pragma unroll
  for (int r = 0; r < N; ++r) x0[r] = 0;
  bool reinit = false;
  if (cand) {
    const T* meas = static_cast<const T*>(a.meas);
    T p7[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) p7[c] = meas[(long)c * a.meas_ld + e];
    if constexpr (M::ANGULAR) {
      T p6[6];
      pose7_to_pose6(p7, p6);
#pragma unroll
      for (int c = 0; c < 6; ++c) x0[c] = p6[c];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) x0[c] = p7[c];
    }
    reinit = true;
#pragma unroll
    for (int r = 0; r < C::K; ++r) reinit = reinit && (x0[r] - x0[r] == (T)0);   // finite
    if (reinit) { ev = (unsigned char)(0x80u | c1); run = 0; }
  }
  if (store_run) a.run[e] = run;
  if (valid && a.event != nullptr) a.event[e] = ev;
  if (__ballot(reinit) == 0ull) return;
  if constexpr (C::UT) {
    static_assert(C::TPW == 64 && kReacquireBlock % 64 == 0, "a wavefront is one tile");
    if (a.tile_uni != nullptr) {
      const long tile = e / C::TPW;   // (the same in every lane of the wavefront)
      if (a.tile_uni[tile] != 0) {
        if (valid)
          for (int k = 0; k < C::LW; ++k)
            *reinterpret_cast<T*>(a.rec + tile * C::TILE_BYTES + record_word_offset<C, T>((int)(e % C::TPW), C::LIN.w[k])) = (T)a.tile_blk[tile * C::LW + k];
        if ((threadIdx.x & 63) == 0) a.tile_uni[tile] = 0;
      }
    }
  }
  if (!reinit) return;
  const double* P0 = a.p0_tab + (long)a.p0_idx[e] * N * N;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    state_set<C, T>(a.rec, e, r, N, x0[r]);
    for (int c = ((C::PK || C::SEPPK) ? r : 0); c < N; ++c) state_set<C, T>(a.rec, e, r, c, (T)P0[r * N + c]);
  }
  if constexpr (M::ANGULAR) {
    for (int cc = 0; cc < 3; ++cc) *unwrap_ptr<C, T>(a.rec, e, cc) = 0;
  }
}

template <class M, typename T, int G, int LAYOUT>
void launch_reacquire(const ReacquireArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((reacquire_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + kReacquireBlock - 1) / kReacquireBlock)), dim3(kReacquireBlock), 0, s, a);
}

#define TE_REACQUIRE_INSTANCE(M, T, G, LAYOUT) template void launch_reacquire<M, T, G, LAYOUT>(const ReacquireArgs&, hipStream_t);
// the layouts every model has in both precisions
#define TE_REACQUIRE_COMMON(M)                                   \
  TE_REACQUIRE_INSTANCE(M, double, 3, LAYOUT_FULL)               \
  TE_REACQUIRE_INSTANCE(M, double, 3, LAYOUT_PACKED)             \
  TE_REACQUIRE_INSTANCE(M, double, 1, LAYOUT_SEPARABLE)          \
  TE_REACQUIRE_INSTANCE(M, double, 1, LAYOUT_SEPARABLE_PACKED)   \
  TE_REACQUIRE_INSTANCE(M, double, 1, LAYOUT_SEPARABLE_SHARED)   \
  TE_REACQUIRE_INSTANCE(M, float, 3, LAYOUT_FULL)                \
  TE_REACQUIRE_INSTANCE(M, float, 3, LAYOUT_PACKED)              \
  TE_REACQUIRE_INSTANCE(M, float, 1, LAYOUT_SEPARABLE)           \
  TE_REACQUIRE_INSTANCE(M, float, 1, LAYOUT_SEPARABLE_PACKED)

}  // namespace te
