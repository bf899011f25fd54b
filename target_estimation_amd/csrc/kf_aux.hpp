// kf_aux.hpp -- record access, target construction and output derivation kernels.
// Not bandwidth-critical (one thread per target or per row); the step kernel is kf_step.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "te_clock.hpp"
#include "te_device_math.hpp"
#include "te_layout.hpp"
#include "te_quartic.hpp"

namespace te {

// pointer to element (r, c) of P (c < N) or to x[r] (c == N) of `slot`; nullptr for a
// structurally zero element of the separable layout
template <class C, typename T>
__device__ __forceinline__ T* state_ptr(char* rec, long slot, int r, int c) {
  const long tile = slot / C::TPW;
  const int lane = (int)(slot % C::TPW) * C::G + ((c >= C::N) ? (r % C::G) : C::p_lane(r, c));
  const int q = (r % C::K) / C::G + (r / C::K) * C::KPL;
  const int w = (c >= C::N) ? C::X_OFF + q : C::p_word(r, c);
  if (w < 0) return nullptr;
  return reinterpret_cast<T*>(rec + tile * C::TILE_BYTES + record_word_offset<C, T>(lane, w));
}
template <class C, typename T>
__device__ __forceinline__ T state_get(char* rec, long slot, int r, int c) {
  const T* p = state_ptr<C, T>(rec, slot, r, c);
  return p ? *p : (T)0;
}
template <class C, typename T>
__device__ __forceinline__ void state_set(char* rec, long slot, int r, int c, T v) {
  T* p = state_ptr<C, T>(rec, slot, r, c);
  if (p) *p = v;
}
// pointer to unwrap-memory component cc (0..2) of `slot`
template <class C, typename T>
__device__ __forceinline__ T* unwrap_ptr(char* rec, long slot, int cc) {
  const int r = 3 + cc;
  const long tile = slot / C::TPW;
  const int lane = (int)(slot % C::TPW) * C::G + (r % C::G);
  const int w = C::UW_OFF + cc / C::G;
  return reinterpret_cast<T*>(rec + tile * C::TILE_BYTES + record_word_offset<C, T>(lane, w));
}

// geometry.hpp:619-628 pose7dToPose6d
template <typename T> __device__ __forceinline__ void pose7_to_pose6(const T* p7, T* p6) {
  T q[4] = {p7[3], p7[4], p7[5], p7[6]};
  p6[0] = p7[0]; p6[1] = p7[1]; p6[2] = p7[2];
  quat_normalize(q);
  quat_to_rpy(q, p6 + 3);
}

struct InitArgs {
  char* rec;
  const int* idx;          // slot of entry e
  long n;
  const double* p0;        // [n][7]
  const double* v0;        // [n][6] or null
  const double* a0;        // [n][6] or null
  const double* P0;        // [N*N] shared, [n][N*N] when per_target_P0, or a table indexed by P0_index
  int per_target_P0;
  const int* P0_index = nullptr;   // [n]: entry e starts from P0 + P0_index[e] * N*N (per-class initial covariances)
  int* cls = nullptr;              // per-slot parameter class array of the batch
  const int* cls_of = nullptr;     // [n] class of entry e, or null: every entry gets cls_value
  int cls_value = 0;
  TClock t_off;            // t0 - batch clock
  int nm_off;              // - batch measurement counter
  TClock* t_base;
  int* nm_base;
};

// Model constructors: uniform_velocity.cpp:50-56, uniform_acceleration.cpp:50-57,
// angular_rates.cpp:57-65, angular_velocities.cpp:51-56,73 + KalmanFilterInterface::init
// src/kalman.cpp:16-21 (x = x0, P = P0).  The unwrap memory starts at zero (the reference
// leaves meas_rpy_internal_ uninitialised: angular_rates.hpp:110, angular_velocities.hpp:127).
template <class M, typename T, int G, int LAYOUT>
__global__ void init_kernel(const InitArgs a) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const long slot = a.idx[e];
  T p7[7], x0[N];
#pragma unroll
  for (int c = 0; c < 7; ++c) p7[c] = (T)a.p0[e * 7 + c];
#pragma unroll
  for (int r = 0; r < N; ++r) x0[r] = 0;
  T v6[6], a6[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) { v6[c] = a.v0 ? (T)a.v0[e * 6 + c] : (T)0; a6[c] = a.a0 ? (T)a.a0[e * 6 + c] : (T)0; }
  if constexpr (M::TYPE == UNIFORM_VELOCITY) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { x0[c] = p7[c]; x0[3 + c] = v6[c]; }
  } else if constexpr (M::TYPE == UNIFORM_ACCELERATION) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { x0[c] = p7[c]; x0[3 + c] = v6[c]; x0[6 + c] = a6[c]; }
  } else {
    T p6[6];
    pose7_to_pose6(p7, p6);
#pragma unroll
    for (int c = 0; c < 6; ++c) { x0[c] = p6[c]; x0[6 + c] = v6[c]; }
    if constexpr (M::TYPE == ANGULAR_RATES) {
#pragma unroll
      for (int c = 0; c < 6; ++c) x0[12 + c] = a6[c];
    }
  }
  const double* P0 = a.P0 + (a.P0_index ? (long)a.P0_index[e] * N * N : (a.per_target_P0 ? e * N * N : 0));
  if (a.cls) a.cls[slot] = a.cls_of ? a.cls_of[e] : a.cls_value;
  for (int r = 0; r < N; ++r) {
    state_set<C, T>(a.rec, slot, r, N, x0[r]);
    for (int c = ((C::PK || C::SEPPK) ? r : 0); c < N; ++c) state_set<C, T>(a.rec, slot, r, c, (T)P0[r * N + c]);
  }
  if constexpr (M::ANGULAR) {
    for (int cc = 0; cc < 3; ++cc) *unwrap_ptr<C, T>(a.rec, slot, cc) = 0;
  }
  a.t_base[slot] = a.t_off;
  a.nm_base[slot] = a.nm_off;
}

// x [n][N] and P [n][N*N] (row-major, doubles) of the listed slots; one thread per (entry,row)
// tile_uni / tile_blk (or null): the batch's uniform tiles (te_layout.hpp Cfg::UT) -- the linear P words of a flagged tile are
// read from the tile's block.  Read-only: a caller that polls the state does not end a tile's uniformity.
template <class M, typename T, int G, int LAYOUT>
__global__ void get_state_kernel(char* rec, const int* idx, long n, double* x_out, double* P_out, const double* tile_blk, const int* tile_uni) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= n * N) return;
  const long e = tid / N;
  const int r = (int)(tid % N);
  const long slot = idx ? (long)idx[e] : e;
  if (x_out) x_out[e * N + r] = (double)state_get<C, T>(rec, slot, r, N);
  if (!P_out) return;
  bool uni = false;
  if constexpr (C::UT) uni = tile_uni != nullptr && tile_uni[slot / C::TPW] != 0;
  for (int c = 0; c < N; ++c) {
    double v = (double)state_get<C, T>(rec, slot, r, c);
    if constexpr (C::UT) {
      const int w = C::PWORD.v[r][c];
      if (uni && w >= 0 && C::LIN.idx[w] >= 0) v = tile_blk[(slot / C::TPW) * C::LW + C::LIN.idx[w]];
    }
    P_out[(e * N + r) * N + c] = v;
  }
}

// Uniform tiles: the block of every flagged tile back into the linear P words of its lanes' records (thread per target).  After
// it, and with the flags cleared behind it, the records alone are the state again: what every launch that is not a dense tick
// of the form expects (Batch::settle_tiles).  A copy: exact.
template <class M, typename T>
__global__ void settle_tiles_kernel(char* rec, long n, const double* tile_blk, const int* tile_uni) {
  using C = Cfg<M, T, 1, LAYOUT_SEPARABLE_SHARED>;
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n) return;
  const long tile = slot / C::TPW;
  if (tile_uni[tile] == 0) return;
  for (int k = 0; k < C::LW; ++k)
    *reinterpret_cast<T*>(rec + tile * C::TILE_BYTES + record_word_offset<C, T>((int)(slot % C::TPW), C::LIN.w[k])) = (T)tile_blk[tile * C::LW + k];
}

template <class M, typename T, int G, int LAYOUT>
__global__ void set_state_kernel(char* rec, const int* idx, long n, const double* x_in, const double* P_in,
                                 const double* uw_in) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= n * N) return;
  const long e = tid / N;
  const int r = (int)(tid % N);
  const long slot = idx ? (long)idx[e] : e;
  if (x_in) state_set<C, T>(rec, slot, r, N, (T)x_in[e * N + r]);
  if (P_in)
    for (int c = ((C::PK || C::SEPPK) ? r : 0); c < N; ++c) state_set<C, T>(rec, slot, r, c, (T)P_in[(e * N + r) * N + c]);
  if constexpr (M::ANGULAR) {
    if (uw_in && r < 3) *unwrap_ptr<C, T>(rec, slot, r) = (T)uw_in[e * 3 + r];
  }
}

// copy the whole record of slot `src` over slot `dst` (erase = swap-with-last compaction)
template <class M, typename T, int G, int LAYOUT>
__global__ void move_record_kernel(char* rec, long src, long dst, TClock* t_base, int* nm_base, int* cls) {
  using C = Cfg<M, T, G, LAYOUT>;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= C::G * C::RW) return;
  const int i = tid / C::RW, w = tid % C::RW;
  const T v = *reinterpret_cast<T*>(rec + (src / C::TPW) * C::TILE_BYTES +
                                    record_word_offset<C, T>((int)(src % C::TPW) * C::G + i, w));
  *reinterpret_cast<T*>(rec + (dst / C::TPW) * C::TILE_BYTES +
                        record_word_offset<C, T>((int)(dst % C::TPW) * C::G + i, w)) = v;
  if (tid == 0) { t_base[dst] = t_base[src]; nm_base[dst] = nm_base[src]; if (cls) cls[dst] = cls[src]; }
}

// m independent moves at once (batched erase: survivors from the tail fill the holes); blockIdx.y = move
template <class M, typename T, int G, int LAYOUT>
__global__ void move_records_kernel(char* rec, const int* src, const int* dst, long m, TClock* t_base, int* nm_base, int* cls) {
  using C = Cfg<M, T, G, LAYOUT>;
  const long mv = blockIdx.y;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (mv >= m || tid >= C::G * C::RW) return;
  const long s = src[mv], d = dst[mv];
  const int i = tid / C::RW, w = tid % C::RW;
  const T v = *reinterpret_cast<T*>(rec + (s / C::TPW) * C::TILE_BYTES + record_word_offset<C, T>((int)(s % C::TPW) * C::G + i, w));
  *reinterpret_cast<T*>(rec + (d / C::TPW) * C::TILE_BYTES + record_word_offset<C, T>((int)(d % C::TPW) * C::G + i, w)) = v;
  if (tid == 0) { t_base[d] = t_base[s]; nm_base[d] = nm_base[s]; if (cls) cls[d] = cls[s]; }
}

// A batch in the shared-axes storage form (te_layout.hpp) leaves it: slot by slot, x, the unwrap memory and every stored word of
// P of the plain LAYOUT_SEPARABLE_PACKED record, read from the shared record (whose p_word maps every axis of a kind to the
// kind's one block).  A copy: exact.  Once per batch at most, thread per target.
template <class M, typename T>
__global__ void expand_shared_kernel(char* rec, char* rec_plain, long n) {
  using CS = Cfg<M, T, 1, LAYOUT_SEPARABLE_SHARED>;
  using CP = Cfg<M, T, 1, LAYOUT_SEPARABLE_PACKED>;
  constexpr int N = CS::N;
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n) return;
  for (int r = 0; r < N; ++r) {
    state_set<CP, T>(rec_plain, slot, r, N, state_get<CS, T>(rec, slot, r, N));
    for (int c = r; c < N; ++c) state_set<CP, T>(rec_plain, slot, r, c, state_get<CS, T>(rec, slot, r, c));   // (no-op between groups)
  }
  if constexpr (M::ANGULAR) {
    for (int cc = 0; cc < 3; ++cc) *unwrap_ptr<CP, T>(rec_plain, slot, cc) = *unwrap_ptr<CS, T>(rec, slot, cc);
  }
}

// measurements: AoS doubles [n][7] (the reference's Vector7d rows) -> SoA T [7][ld]
template <typename T>
__global__ void pack_meas_kernel(const double* aos, long n, T* soa, long ld) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
#pragma unroll
  for (int c = 0; c < 7; ++c) soa[c * ld + e] = (T)aos[e * 7 + c];
}

struct OutArgs {
  char* rec;
  const int* idx;   // null: dense slots 0..n-1
  long n;
  double* pose;     // [n][7] or null
  double* twist;    // [n][6] or null
  double* acc;      // [n][6] or null
  int at_time;      // 0: current outputs; 1: extrapolated to t1 (getEstimated*(t1))
  double t1;        // absolute query time (at_time); NaN = each target's own time
  TClock t_acc;     // batch clock; target time = t_base[slot] + t_acc (te_clock.hpp)
  const TClock* t_base;
  int by_slot = 0;  // 1: output row = slot (scatter into a per-slot table) instead of the entry index
  // One-workgroup launches only (n <= kOutputsBlock): after every row has been written, store done_seq to *done_flag
  // (host-mapped memory).  A host thread that spins on the flag sees the rows without a stream synchronisation: the
  // one-target ABI's round trip is a launch and a PCIe write instead of a launch and the runtime's completion path.
  int* done_flag = nullptr;
  int done_seq = 0;
  // pose_soa (or null): the poses once more, SoA [7][pose_ld] (column = output row) -- one block of a per-tick pose stream,
  // written by this kernel for the layouts whose step kernel has no pose output of its own (kf_ops_impl.hpp, OpsImpl::step)
  double* pose_soa = nullptr;
  long pose_ld = 0;
  // outputs_rows_kernel only (outputs_kernel never reads it): the destination row of every slot, -1 = none
  const int* row_of_slot = nullptr;
};
constexpr int kOutputsBlock = 128;

// Derived outputs of one target, from x only.
//  current : updateTargetState + getEstimatedPose()/Twist()/Acceleration()
//            (uniform_velocity.cpp:98-115, uniform_acceleration.cpp:101-118, angular_rates.cpp:117-138,
//             angular_velocities.cpp:153-169, target_interface.cpp:100-115, geometry.hpp:590-608)
//  at t1   : getEstimatedPose(t1)/Twist(t1)/Acceleration(t1)
//            (uniform_velocity.cpp:117-133, uniform_acceleration.cpp:120-136, angular_rates.cpp:140-157,
//             angular_velocities.cpp:171-184, target_interface.cpp:123-140)
template <class M, typename T>
__device__ __forceinline__ void derive_outputs(const T* x, bool at_time, T d, T* pose7, T* twist6, T* acc6) {
#pragma clang fp contract(off)   // the same roundings wherever this is inlined (see te_device_math.hpp)
  T R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  T pint[6] = {x[0], x[1], x[2], 0, 0, 0};  // pose_internal_
#pragma unroll
  for (int c = 0; c < 6; ++c) { twist6[c] = 0; acc6[c] = 0; }
  if constexpr (M::TYPE == UNIFORM_VELOCITY) {
#pragma unroll
    for (int c = 0; c < 3; ++c) twist6[c] = x[3 + c];
  } else if constexpr (M::TYPE == UNIFORM_ACCELERATION) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { twist6[c] = x[3 + c]; acc6[c] = x[6 + c]; }
  } else {
    T q[4];
    rpy_to_quat(x + 3, q);
    quat_to_rot(q, R);
    rot_to_rpy(R, pint + 3);
    if constexpr (M::TYPE == ANGULAR_RATES) {
      // twist.angular = EarBase(rotToRpy(R)) * rates, geometry.hpp:333-351
      T s_r, c_r, s_p, c_p;
      Mth<T>::sincos(pint[3], &s_r, &c_r);
      Mth<T>::sincos(pint[4], &s_p, &c_p);
#pragma unroll
      for (int c = 0; c < 3; ++c) twist6[c] = x[6 + c];
      twist6[3] = (1 * x[9] + 0 * x[10]) + (-s_p) * x[11];
      twist6[4] = (0 * x[9] + c_r * x[10]) + (c_p * s_r) * x[11];
      twist6[5] = (0 * x[9] + (-s_r) * x[10]) + (c_p * c_r) * x[11];
#pragma unroll
      for (int c = 0; c < 6; ++c) acc6[c] = x[12 + c];
    } else {
#pragma unroll
      for (int c = 0; c < 6; ++c) twist6[c] = x[6 + c];
    }
  }
  if (!at_time) {
    pose7[0] = x[0]; pose7[1] = x[1]; pose7[2] = x[2];
    rot_to_quat(R, pose7 + 3);
    return;
  }
  // extrapolation to t1 = t + d
  if constexpr (M::TYPE == UNIFORM_VELOCITY) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pose7[c] = x[c] + twist6[c] * d;
    pose7[3] = 0; pose7[4] = 0; pose7[5] = 0; pose7[6] = 1;
  } else if constexpr (M::TYPE == UNIFORM_ACCELERATION) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pose7[c] = x[c] + twist6[c] * d + (T)0.5 * acc6[c] * d * d;
    pose7[3] = 0; pose7[4] = 0; pose7[5] = 0; pose7[6] = 1;
#pragma unroll
    for (int c = 0; c < 6; ++c) twist6[c] = twist6[c] + acc6[c] * d;
  } else if constexpr (M::TYPE == ANGULAR_RATES) {
    T v6[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) v6[c] = pint[c] + twist6[c] * d + (T)0.5 * acc6[c] * d * d;
    pose7[0] = v6[0]; pose7[1] = v6[1]; pose7[2] = v6[2];
    rpy_to_quat(v6 + 3, pose7 + 3);
    quat_normalize(pose7 + 3);
#pragma unroll
    for (int c = 0; c < 6; ++c) twist6[c] = twist6[c] + acc6[c] * d;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) pose7[c] = x[c] + twist6[c] * d;
    T q0[4];
    rpy_to_quat(pint + 3, q0);
    qtran_apply(d, twist6 + 3, q0, pose7 + 3);
    quat_normalize(pose7 + 3);
  }
}

template <class M, typename T, int G, int LAYOUT>
__global__ void outputs_kernel(const OutArgs a) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long slot = -1;
  if (e < a.n) slot = a.idx ? (long)a.idx[e] : e;   // negative: an entry that is not in this batch (device-resolved ids, id_resolve.hpp)
  if (slot >= 0) {
    T x[N];
#pragma unroll
    for (int r = 0; r < N; ++r) x[r] = state_get<C, T>(a.rec, slot, r, N);
    T d = 0;
    if (a.at_time) d = (a.t1 != a.t1) ? (T)0 : (T)te_clock_offset(a.t1, a.t_base[slot], a.t_acc);
    T pose7[7], twist6[6], acc6[6];
    derive_outputs<M, T>(x, a.at_time != 0, d, pose7, twist6, acc6);
    const long row = a.by_slot ? slot : e;
    if (a.pose) for (int c = 0; c < 7; ++c) a.pose[row * 7 + c] = (double)pose7[c];
    if (a.pose_soa) for (int c = 0; c < 7; ++c) a.pose_soa[(long)c * a.pose_ld + row] = (double)pose7[c];
    if (a.twist) for (int c = 0; c < 6; ++c) a.twist[row * 6 + c] = (double)twist6[c];
    if (a.acc) for (int c = 0; c < 6; ++c) a.acc[row * 6 + c] = (double)acc6[c];
  }
  if (a.done_flag != nullptr) {   // uniform; the launch is one workgroup (OutArgs::done_flag)
    __threadfence_system();       // this thread's rows are visible to the host ...
    __syncthreads();              // ... for every thread of the workgroup ...
    if (threadIdx.x == 0) __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);   // ... before the flag is
  }
}

// getEstimatedPose() of every slot 0..n-1 (derive_outputs, as outputs_kernel) into row a.row_of_slot[slot] of a.pose [rows][7]:
// the ascending-id rows of a whole manager (target_manager_get_est_all_by_id).  A workgroup's rows are staged in LDS and leave
// as one sweep over its 7 * kOutputsBlock doubles, consecutive threads on consecutive doubles of a row, so that a run of
// consecutive ranks is stored as whole 128-byte lines.  A slot whose row is negative stores nothing.
template <class M, typename T, int G, int LAYOUT>
__global__ __launch_bounds__(kOutputsBlock) void outputs_rows_kernel(const OutArgs a) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  __shared__ double s_pose[kOutputsBlock * 7];
  __shared__ int s_row[kOutputsBlock];
  const long e0 = (long)blockIdx.x * kOutputsBlock;
  const long e = e0 + threadIdx.x;
  int row = -1;
  if (e < a.n) {
    row = a.row_of_slot[e];
    if (row >= 0) {
      T x[N];
#pragma unroll
      for (int r = 0; r < N; ++r) x[r] = state_get<C, T>(a.rec, e, r, N);
      T pose7[7], twist6[6], acc6[6];
      derive_outputs<M, T>(x, false, (T)0, pose7, twist6, acc6);
#pragma unroll
      for (int c = 0; c < 7; ++c) s_pose[threadIdx.x * 7 + c] = (double)pose7[c];
    }
  }
  s_row[threadIdx.x] = row;
  __syncthreads();
  const long left = a.n - e0;
  const int cnt = left < kOutputsBlock ? (int)left : kOutputsBlock;
  for (int i = threadIdx.x; i < cnt * 7; i += kOutputsBlock) {
    const int r = i / 7, c = i - r * 7;
    const int dst = s_row[r];
    if (dst >= 0) a.pose[(long)dst * 7 + c] = s_pose[i];
  }
}

// ---- the innovation writer -------------------------------------------------------------------------------------------------
// The innovation stream of a tick (kf_step.hpp StepArgs::nis) for the layouts whose step kernel does not write it itself: the
// dense kf_step_kernel layouts, the symmetric-packed EKF, batches with several (Q, R) classes.  One launch BEFORE the step,
// records read-only: what the step is about to form.
struct InnovArgs {
  char* rec;                       // read, never written (nor is the unwrap memory)
  const void* qr;                  // the batch's [Q | R] row, or (cls != null) its table of rows
  const int* cls;                  // per-slot parameter class, or null
  long n;
  const void* meas;                // SoA [7][meas_ld] in the batch precision, or null (a predict-only tick: sentinels)
  long meas_ld;
  const unsigned char* has_meas;   // per-slot mask or null
  double dt;
  const double* tile_blk;          // the batch's uniform tiles, honoured read-only (null: none)
  const int* tile_uni;
  double* nis;                     // [n]
  double* innov;                   // SoA [m][innov_ld], or null
  long innov_ld;
};

// Thread per target: x^-[0:m] = (A x | f(x))[0:m], S = (A P A^T + Q)[0:m,0:m] + R from the rows of A that reach a measured state
// (src/kalman.cpp:84-92 | :129-137; the EKF's Jacobians at the stored posterior, as the step takes them), S^-1 by unpivoted
// Gauss-Jordan as the step does, y with the unwrapped angles of the angular models, nu = y - x^-[0:m], NIS = nu^T S^-1 nu.  P is
// read element by element through the layout's accessors (state_get, as get_state_kernel): nothing is expanded in memory.
// Off the hot path: correct, not fast.  A target without a measurement gets NIS = -1 and nu = 0.
template <class M, typename T, int G, int LAYOUT>
__global__ void innov_kernel(const InnovArgs a) {
#pragma clang fp contract(off)
  using C = Cfg<M, T, G, LAYOUT>;
  using F = Mth<T>;
  constexpr int N = C::N, K = C::K;   // K = m: the measured states are rows 0..K-1
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const T* meas = static_cast<const T*>(a.meas);
  const bool has = meas != nullptr && (a.has_meas == nullptr || a.has_meas[e] != 0);
  if (!has) {
    a.nis[e] = -1.0;
    if (a.innov != nullptr) for (int c = 0; c < K; ++c) a.innov[(long)c * a.innov_ld + e] = 0.0;
    return;
  }
  const T dt = (T)a.dt, hdt = (T)0.5 * dt * dt;
  const T* qr = static_cast<const T*>(a.qr) + (a.cls ? (long)a.cls[e] * C::QR_WORDS : 0L);
  bool uni = false;
  if constexpr (C::UT) uni = a.tile_uni != nullptr && a.tile_uni[e / C::TPW] != 0;
  auto Pget = [&](int r, int c) -> T {
    if constexpr (C::UT) {
      const int w = C::PWORD.v[r][c];
      if (uni && w >= 0 && C::LIN.idx[w] >= 0) return (T)a.tile_blk[(e / C::TPW) * C::LW + C::LIN.idx[w]];
    }
    return state_get<C, T>(a.rec, e, r, c);
  };
  T x[N];
  for (int r = 0; r < N; ++r) x[r] = state_get<C, T>(a.rec, e, r, N);
  // row r < K of A, sparse: A[r][col[r][j]] = cf[r][j]
  int col[K][6], cnt[K];
  T cf[K][6], xm[K];
  if constexpr (!M::EKF) {
    for (int r = 0; r < K; ++r) {
      col[r][0] = r; cf[r][0] = (T)1;
      col[r][1] = r + K; cf[r][1] = dt;
      cnt[r] = 2;
      xm[r] = F::fma(dt, x[r + K], x[r]);
      if (C::NB == 3) {
        col[r][2] = r + 2 * K; cf[r][2] = hdt;
        cnt[r] = 3;
        xm[r] = F::fma(hdt, x[r + 2 * K], xm[r]);
      }
    }
  } else {
    for (int r = 0; r < 3; ++r) {   // x, y, z: [p v] chains, rows {r, r + 6}
      col[r][0] = r; cf[r][0] = (T)1;
      col[r][1] = r + 6; cf[r][1] = dt;
      cnt[r] = 2;
      xm[r] = F::fma(dt, x[r + 6], x[r]);
    }
    // the attitude rows: geometry.hpp:394-426 (Jacobians at the stored posterior), :359-374 (EarBaseInv), angular_velocities.cpp:137
    T s_r, c_r, s_p, c_p;
    F::sincos(x[3], &s_r, &c_r);
    F::sincos(x[4], &s_p, &c_p);
    const T wy = x[10], wz = x[11];
    T Jr[3][3], Jw[3][3], Ei[3][3];
    Jr[0][0] = (dt * (wy * c_r * s_p - wz * s_p * s_r)) / c_p + 1;
    Jr[0][1] = (dt * (wz * c_r + wy * s_r)) / (c_p * c_p);
    Jr[0][2] = 0;
    Jr[1][0] = -dt * (wz * c_r + wy * s_r);
    Jr[1][1] = 1;
    Jr[1][2] = 0;
    Jr[2][0] = (dt * (wy * c_r - wz * s_r)) / c_p;
    Jr[2][1] = (dt * s_p * (wz * c_r + wy * s_r)) / (c_p * c_p);
    Jr[2][2] = 1;
    Jw[0][0] = dt; Jw[0][1] = (dt * s_p * s_r) / c_p; Jw[0][2] = (dt * c_r * s_p) / c_p;
    Jw[1][0] = 0;  Jw[1][1] = dt * c_r;               Jw[1][2] = -dt * s_r;
    Jw[2][0] = 0;  Jw[2][1] = (dt * s_r) / c_p;       Jw[2][2] = (dt * c_r) / c_p;
    Ei[0][0] = 1; Ei[0][1] = (s_p * s_r) / c_p; Ei[0][2] = (c_r * s_p) / c_p;
    Ei[1][0] = 0; Ei[1][1] = c_r;               Ei[1][2] = -s_r;
    Ei[2][0] = 0; Ei[2][1] = s_r / c_p;         Ei[2][2] = c_r / c_p;
    for (int r = 0; r < 3; ++r) {
      for (int j = 0; j < 3; ++j) {
        col[3 + r][j] = 3 + j; cf[3 + r][j] = Jr[r][j];
        col[3 + r][3 + j] = 9 + j; cf[3 + r][3 + j] = Jw[r][j];
      }
      cnt[3 + r] = 6;
      T acc = (dt * Ei[r][0]) * x[9];
      acc = F::fma(dt * Ei[r][1], x[10], acc);
      acc = F::fma(dt * Ei[r][2], x[11], acc);
      xm[3 + r] = x[3 + r] + acc;
    }
  }
  // S = ((A P) A^T + Q)[0:K,0:K] + R
  T S[K][K];
  for (int r = 0; r < K; ++r)
    for (int c = 0; c < K; ++c) {
      T v = 0;
      for (int j = 0; j < cnt[c]; ++j) {
        T t = 0;   // (A P)[r][col[c][j]]
        for (int i = 0; i < cnt[r]; ++i) t = F::fma(cf[r][i], Pget(col[r][i], col[c][j]), t);
        v = F::fma(t, cf[c][j], v);
      }
      const int qw = C::QWORD.v[r][c], rw = C::RWORD.v[r][c];   // (negative: a structural zero of the separable layouts)
      S[r][c] = (v + (qw >= 0 ? qr[qw] : (T)0)) + (rw >= 0 ? qr[rw] : (T)0);
    }
  // the measurement as the update takes it
  T y[K];
  for (int c = 0; c < 3; ++c) y[c] = meas[(long)c * a.meas_ld + e];
  if constexpr (M::ANGULAR) {
    T q[4], mrpy[3];
    for (int c = 0; c < 4; ++c) q[c] = meas[(long)(3 + c) * a.meas_ld + e];
    quat_normalize(q);
    quat_to_rpy(q, mrpy);
    for (int c = 0; c < 3; ++c) y[3 + c] = unwrap_angle(*unwrap_ptr<C, T>(a.rec, e, c), mrpy[c]);   // (read only)
  }
  T nu[K];
  for (int c = 0; c < K; ++c) nu[c] = y[c] - xm[c];
  for (int p = 0; p < K; ++p) {   // unpivoted Gauss-Jordan (S is SPD), as the step kernels
    const T inv = (T)1 / S[p][p];
    S[p][p] = 1;
    for (int c = 0; c < K; ++c) S[p][c] *= inv;
    for (int r = 0; r < K; ++r) {
      if (r == p) continue;
      const T f = S[r][p];
      S[r][p] = 0;
      for (int c = 0; c < K; ++c) S[r][c] = F::fma(-f, S[p][c], S[r][c]);
    }
  }
  T nis = 0;
  for (int r = 0; r < K; ++r) {
    T w = 0;
    for (int c = 0; c < K; ++c) w = F::fma(S[r][c], nu[c], w);
    nis = F::fma(nu[r], w, nis);
  }
  a.nis[e] = (double)nis;
  if (a.innov != nullptr) for (int c = 0; c < K; ++c) a.innov[(long)c * a.innov_ld + e] = (double)nu[c];
}

// The effective mask of a gated tick whose layout has no gated step kernel (StepParams::gate_row), from the NIS row the writer
// above has just written: has_eff[e] = has && nis[e] <= gate -- the double of the stream, so a NaN rejects.  The step that follows
// takes the row as its has_meas.  A launch of its own behind the writer, which stays the code it was.  (A template only so that
// every translation unit that launches it may hold it.)
template <typename Tag = void>
__global__ void gate_mask_kernel(const double* nis, const unsigned char* has_meas, int measured, long n, double gate, unsigned char* has_eff) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const bool has = measured != 0 && (has_meas == nullptr || has_meas[e] != 0);
  has_eff[e] = (has && nis[e] <= gate) ? 1 : 0;
}

struct IntersectArgs {
  char* rec;
  const int* idx;     // null: dense slots 0..n-1
  long n;
  double t1;          // absolute query time; NaN = each target's own time (t1 = t_)
  double origin[3];
  double radius;
  TClock t_acc;
  const TClock* t_base;
  double* delta;      // [n]: time to the first intersection after t1, or -1
  double* pose;       // [n][7] pose at t1 + delta (initPose if none), or null
};

// IntersectionSolver::getIntersectionTimeWithSphere / getIntersectionPoseWithSphere without the
// moving-average convergence gate (src/intersection_solver.cpp:42-104) for one target with state x:
// quartic in delta from the (p, v, a) extrapolated by dq = t1 - t_, smallest real root, pose at
// t1 + delta, i.e. at the offset delta + dq (the reference's (delta + t1) - t_, with the clock's
// offset taken before t1's rounding).  own = the query is at the target's own time (dq = 0).
// The values: delta (the reference's intersection time, -1 if none) and, if wanted, the pose at that time (identity if none).
template <class M, typename T>
__device__ __forceinline__ void sphere_query_values(const T* x, bool own, double dq, const double* origin, double radius,
                                                    double& delta, double (&pose)[7], const bool want_pose
#ifdef TE_QUERY_PHASE_CLOCK
                                                    , long long* ts = nullptr
#endif
                                                    ) {
#pragma clang fp contract(off)   // fused query, intersect kernel: the same roundings (te_device_math.hpp)
#ifdef TE_QUERY_PHASE_CLOCK
#define TE_TS(i) do { if (ts) { __builtin_amdgcn_sched_barrier(0); ts[i] = (long long)__builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define TE_TS(i) do {} while (0)
#endif
  T pose7[7], twist6[6], acc6[6];
  derive_outputs<M, T>(x, true, own ? (T)0 : (T)dq, pose7, twist6, acc6);
  const double px = (double)pose7[0] - origin[0], py = (double)pose7[1] - origin[1], pz = (double)pose7[2] - origin[2];
  const double vx = (double)twist6[0], vy = (double)twist6[1], vz = (double)twist6[2];
  const double ax = (double)acc6[0], ay = (double)acc6[1], az = (double)acc6[2];
  double c[5];
  c[4] = 0.25 * (ax * ax + ay * ay + az * az);
  c[3] = vx * ax + vy * ay + vz * az;
  c[2] = vx * vx + vy * vy + vz * vz + px * ax + py * ay + pz * az;
  c[1] = 2 * (px * vx + py * vy + pz * vz);
  c[0] = px * px + py * py + pz * pz - radius * radius;
  TE_TS(1);
  const double d = first_crossing_quartic(c);   // leftmost real root if >= 0, else -1
  TE_TS(2);
  delta = d;
  // (the array is taken by reference and the choice is a flag: a pointer that may be null made the caller's array escape into
  // scratch memory -- 64 bytes per lane, and a resident kernel with scratch is also limited by the process's scratch wave slots)
  if (want_pose) {
    pose[0] = pose[1] = pose[2] = pose[3] = pose[4] = pose[5] = 0; pose[6] = 1;
    if (d > -1) {
      derive_outputs<M, T>(x, true, own ? (T)d : (T)(d + dq), pose7, twist6, acc6);
#pragma unroll
      for (int k = 0; k < 7; ++k) pose[k] = (double)pose7[k];
    }
  }
  TE_TS(3);
}

template <class M, typename T>
__device__ __forceinline__ void sphere_query(const T* x, bool own, double dq, const double* origin, double radius,
                                             double* delta_out, double* pose_out /* [7] or null */) {
  double d, out[7];
  sphere_query_values<M, T>(x, own, dq, origin, radius, d, out, pose_out != nullptr);
  *delta_out = d;
  if (pose_out)
    for (int k = 0; k < 7; ++k) pose_out[k] = out[k];
}

template <class M, typename T, int G, int LAYOUT>
__global__ void intersect_kernel(const IntersectArgs a) {
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const long slot = a.idx ? (long)a.idx[e] : e;
  T x[N];
#pragma unroll
  for (int r = 0; r < N; ++r) x[r] = state_get<C, T>(a.rec, slot, r, N);
  // own-time query (t1 = NaN): the offsets are 0 and delta themselves, so a recorded launch (hipGraph)
  // does not depend on the batch clock; the reference's (delta + t1) - t_ differs by at most ulp(t_)
  const bool own = a.t1 != a.t1;
  const double dq = own ? 0.0 : te_clock_offset(a.t1, a.t_base[slot], a.t_acc);
  sphere_query<M, T>(x, own, dq, a.origin, a.radius, &a.delta[e], a.pose ? &a.pose[e * 7] : nullptr);
}

}  // namespace te
