// kf_step_sep.hpp -- predict+update for axis-separable batches (LAYOUT_SEPARABLE).
//
// When Q, R and P0 have no entries between different axis groups (te_layout.hpp, group_of) the
// dense filter of src/kalman.cpp:84-95 / :129-140 never creates any: every product that would
// touch such an entry multiplies an exact zero.  The step below is therefore the SAME arithmetic
// as kf_step.hpp with the structurally zero terms left out:
//   linear models : one [p v (a)] filter with a scalar measurement per axis
//                   (uniform_velocity 3 x 2 states, uniform_acceleration 3 x 3, angular_rates 6 x 3);
//   EKF           : three [p v] filters for x, y, z and one 6-state [rpy, omega] EKF with the
//                   3-vector Euler-angle measurement (Jacobians of angular_velocities.cpp:116-124).
// Per target the record shrinks from n^2 + n to sum(group^2) + n words (angular_rates: 345 -> 75),
// which is what makes this worth a kernel: the step is HBM-bound.  Thread per target, everything
// in registers, no LDS; Q and R are read through the scalar cache (uniform addresses).
// The host only selects this layout after checking the matrices (target_manager.cpp,
// is_axis_separable); general matrices use the dense kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "kf_aux.hpp"
#include "kf_step.hpp"

namespace te {

// one [p v (a)] chain with a scalar position measurement: rows r0, r0+K, r0+2K of the model
// INNOV: also hands out what the innovation stream needs, the chain's 1 / S (inv_out) and its innovation y - x^-_0 (nu_out): the
// values the gain and the state update use, not second ones.  Untouched without a measurement.
template <int NB, typename T, bool INNOV = false>
__device__ __forceinline__ void sep_linear_axis(T* x, T (&P)[NB][NB], const T (&Q)[NB][NB], T r_meas, T dt, bool has, T y,
                                                T* inv_out = nullptr, T* nu_out = nullptr) {
#pragma clang fp contract(off)  // only the explicit fma calls fuse: same roundings as the dense kernel
  using F = Mth<T>;
  const T hdt = (T)0.5 * dt * dt;
  // x^- = A x ; AP = A P (rows)
#pragma unroll
  for (int b = 0; b + 1 < NB; ++b) {
    x[b] = F::fma(dt, x[b + 1], x[b]);
    if (NB == 3 && b == 0) x[b] = F::fma(hdt, x[b + 2], x[b]);
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      T v = F::fma(dt, P[b + 1][c], P[b][c]);
      if (NB == 3 && b == 0) v = F::fma(hdt, P[b + 2][c], v);
      P[b][c] = v;
    }
  }
  // (AP) A^T (columns), + Q
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      T v = P[b][c];
      if (c + 1 < NB) {
        v = F::fma(dt, P[b][c + 1], v);
        if (NB == 3 && c == 0) v = F::fma(hdt, P[b][c + 2], v);
      }
      P[b][c] = v + Q[b][c];
    }
  if (!has) return;
  // S = P00 + R ; K = P[:,0] / S ; x += K (y - x0) ; P = (I - K C) P
  const T inv = (T)1 / (P[0][0] + r_meas);
  T Kg[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) Kg[b] = P[b][0] * inv;
  const T nu = y - x[0];
  if constexpr (INNOV) { *inv_out = inv; *nu_out = nu; }
#pragma unroll
  for (int b = 0; b < NB; ++b) x[b] += Kg[b] * nu;
  T top[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) top[c] = P[0][c];
  const T d0 = (T)1 - Kg[0];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    P[0][c] = d0 * top[c];
#pragma unroll
    for (int b = 1; b < NB; ++b) {
      const T t = ((T)0 - Kg[b]) * top[c];
      P[b][c] = t + P[b][c];
    }
  }
}

// The same step as two halves that meet only in the gain Kg, for batches in the shared-axes storage form (te_layout.hpp,
// share_rep), which run the covariance half once per KIND of axis and the state half per axis with the kind's Kg:
//   sep_linear_cov   : P^- = A P A^T + Q, and with a measurement S^-1, Kg = P^-[:,0] / S, P = (I - Kg C) P^-.  Reads P, Q, R, dt
//                      and `has` -- never x or the measurement.
//   sep_linear_state : x^- = A x, and with a measurement x += Kg (y - x0).
// Operation for operation the statements of sep_linear_axis above, which stays as it is for every other batch: the register
// allocation of the kernels that sit at an occupancy limit follows its statement order (built from the halves, the per-class
// angular_rates fp64 kernels spilled 116 B per lane and the resident ones lost a wavefront per SIMD).  tests/test_gpu_shared_axes.py
// holds the two forms to the same bits.
// INNOV: sep_linear_cov hands out its 1 / S (one per kind of axis), sep_linear_state its innovation (one per axis), as above.
template <int NB, typename T, bool INNOV = false>
__device__ __forceinline__ void sep_linear_cov(T (&P)[NB][NB], const T (&Q)[NB][NB], T r_meas, T dt, bool has, T (&Kg)[NB], T* inv_out = nullptr) {
#pragma clang fp contract(off)  // only the explicit fma calls fuse: same roundings as the dense kernel
  using F = Mth<T>;
  const T hdt = (T)0.5 * dt * dt;
  // AP = A P (rows)
#pragma unroll
  for (int b = 0; b + 1 < NB; ++b) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      T v = F::fma(dt, P[b + 1][c], P[b][c]);
      if (NB == 3 && b == 0) v = F::fma(hdt, P[b + 2][c], v);
      P[b][c] = v;
    }
  }
  // (AP) A^T (columns), + Q
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      T v = P[b][c];
      if (c + 1 < NB) {
        v = F::fma(dt, P[b][c + 1], v);
        if (NB == 3 && c == 0) v = F::fma(hdt, P[b][c + 2], v);
      }
      P[b][c] = v + Q[b][c];
    }
#pragma unroll
  for (int b = 0; b < NB; ++b) Kg[b] = (T)0;   // (unused without a measurement)
  if (!has) return;
  // S = P00 + R ; K = P[:,0] / S ; P = (I - K C) P
  const T inv = (T)1 / (P[0][0] + r_meas);
  if constexpr (INNOV) *inv_out = inv;
#pragma unroll
  for (int b = 0; b < NB; ++b) Kg[b] = P[b][0] * inv;
  T top[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) top[c] = P[0][c];
  const T d0 = (T)1 - Kg[0];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    P[0][c] = d0 * top[c];
#pragma unroll
    for (int b = 1; b < NB; ++b) {
      const T t = ((T)0 - Kg[b]) * top[c];
      P[b][c] = t + P[b][c];
    }
  }
}

template <int NB, typename T, bool INNOV = false>
__device__ __forceinline__ void sep_linear_state(T* x, T dt, bool has, T y, const T (&Kg)[NB], T* nu_out = nullptr) {
#pragma clang fp contract(off)
  using F = Mth<T>;
  const T hdt = (T)0.5 * dt * dt;
  // x^- = A x
#pragma unroll
  for (int b = 0; b + 1 < NB; ++b) {
    x[b] = F::fma(dt, x[b + 1], x[b]);
    if (NB == 3 && b == 0) x[b] = F::fma(hdt, x[b + 2], x[b]);
  }
  if (!has) return;
  // x += K (y - x0)
  const T nu = y - x[0];
  if constexpr (INNOV) *nu_out = nu;
#pragma unroll
  for (int b = 0; b < NB; ++b) x[b] += Kg[b] * nu;
}

// GATE (sep_step_wave): the same statements once more, cut where the validation gate decides -- between the prediction and the
// update, for ALL chains of a target.  Statement for statement the halves of sep_linear_axis (and of sep_linear_cov /
// sep_linear_state, whose statements are the same ones): the gated kernels are held to the bits of the plain ones
// (tests/test_gpu_gate.py).
//   sep_gate_predict_x / sep_gate_predict_P : x^- = A x / P^- = A P A^T + Q -- what precedes `if (!has) return`
//   sep_gate_gain, sep_gate_update_x / _P   : what follows it, with the 1 / S and nu formed at the decision: the gain from the
//                                             column P^-[:,0] as predicted (P^-[b][0] and P^-[0][b] round differently, and a
//                                             packed record keeps the upper triangle only), then the state half (per axis) and
//                                             the covariance half (per chain; per kind of axis in the shared-axes form).
template <int NB, typename T>
__device__ __forceinline__ void sep_gate_predict_x(T* x, T dt) {
#pragma clang fp contract(off)
  using F = Mth<T>;
  const T hdt = (T)0.5 * dt * dt;
#pragma unroll
  for (int b = 0; b + 1 < NB; ++b) {
    x[b] = F::fma(dt, x[b + 1], x[b]);
    if (NB == 3 && b == 0) x[b] = F::fma(hdt, x[b + 2], x[b]);
  }
}
template <int NB, typename T>
__device__ __forceinline__ void sep_gate_predict_P(T (&P)[NB][NB], const T (&Q)[NB][NB], T dt) {
#pragma clang fp contract(off)
  using F = Mth<T>;
  const T hdt = (T)0.5 * dt * dt;
  // AP = A P (rows)
#pragma unroll
  for (int b = 0; b + 1 < NB; ++b) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      T v = F::fma(dt, P[b + 1][c], P[b][c]);
      if (NB == 3 && b == 0) v = F::fma(hdt, P[b + 2][c], v);
      P[b][c] = v;
    }
  }
  // (AP) A^T (columns), + Q
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      T v = P[b][c];
      if (c + 1 < NB) {
        v = F::fma(dt, P[b][c + 1], v);
        if (NB == 3 && c == 0) v = F::fma(hdt, P[b][c + 2], v);
      }
      P[b][c] = v + Q[b][c];
    }
}
template <int NB, typename T>
__device__ __forceinline__ void sep_gate_gain(const T (&pcol)[NB], T inv, T (&Kg)[NB]) {
#pragma clang fp contract(off)
  // K = P^-[:,0] / S
#pragma unroll
  for (int b = 0; b < NB; ++b) Kg[b] = pcol[b] * inv;
}
template <int NB, typename T>
__device__ __forceinline__ void sep_gate_update_x(T* x, const T (&Kg)[NB], T nu) {
#pragma clang fp contract(off)
  // x += K (y - x0)
#pragma unroll
  for (int b = 0; b < NB; ++b) x[b] += Kg[b] * nu;
}
template <int NB, typename T>
__device__ __forceinline__ void sep_gate_update_P(T (&P)[NB][NB], const T (&Kg)[NB]) {
#pragma clang fp contract(off)
  // P = (I - K C) P
  T top[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) top[c] = P[0][c];
  const T d0 = (T)1 - Kg[0];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    P[0][c] = d0 * top[c];
#pragma unroll
    for (int b = 1; b < NB; ++b) {
      const T t = ((T)0 - Kg[b]) * top[c];
      P[b][c] = t + P[b][c];
    }
  }
}

// Uniform tiles (te_layout.hpp Cfg::UT): a record in two parts -- its linear-covariance chunks (LIN), which a uniform tile neither
// loads nor stores, and everything else (the other chunks and the tail row).
// PART (kf_step.hpp RecPart): of that part, the chunks that hold x / unwrap words, or the others.
template <class C, typename T, bool LIN, int PART = kRecAll>
__device__ __forceinline__ void load_record_part(const char* tb, int lane, T* rec) {
  static_assert(sizeof(T) == 8 && C::REM2 == 0, "the shared-axes form is fp64");
#pragma unroll
  for (int c = 0; c < C::NC; ++c) {
    if (C::lin_chunk(c) != LIN || !rec_part_has<C>(PART, c)) continue;
    const double2 v = *reinterpret_cast<const double2*>(tb + (long)c * C::LPT * 16 + (long)lane * 16);
    rec[c * 2] = v.x; rec[c * 2 + 1] = v.y;
  }
  if constexpr (C::REM1 && !LIN && PART != kRecCov) rec[C::RW - 1] = *reinterpret_cast<const T*>(tb + C::TAIL1_OFF + (long)lane * (long)sizeof(T));
}

// The order of a wavefront's loads in a launched dense single tick (sep_step_wave, MF): the tile flag, then the measurement words
// and the has-byte, then the record's x / unwrap chunks, then its P chunks -- the order in which the tick consumes them.  The
// measurement is the only operand that comes from HBM rather than a cache, and its conversion (quat_normalize, quat_to_rpy) touches
// no record word: requested first, it is waited for alone and converted while the record is still on its way; the EKF group's
// trigonometry, which reads x alone, follows while the P chunks are.  Off for the by-id kernels, the temporally fused loops, the
// resident sessions and the per-class (kPerQR) ticks, which compile to what they were.  -DTE_MEAS_FIRST=0 builds the former order into every kernel, for A/B
// records only (the library is built without it).
// Angular-velocities fp32 on packed groups keeps the former order as well: with the new one every dense kernel of it, and the fp32
// population kernels through their part of it, got 48 B of scratch (profiles/load_order_kernel_resources.txt).
template <class M, typename T, int LAYOUT, unsigned VAR>
constexpr bool sep_meas_first() {
#ifdef TE_MEAS_FIRST
  if (TE_MEAS_FIRST == 0) return false;
#endif
  if (M::TYPE == ANGULAR_VELOCITIES && sizeof(T) == 4 && LAYOUT == LAYOUT_SEPARABLE_PACKED) return false;
  return !sv_has(VAR, kIndexed) && !sv_has(VAR, kFused) && !sv_has(VAR, kPerQR) && sv_live(VAR) == 0;
}
template <class C, typename T, bool NT>
__device__ __forceinline__ void store_record_nonlin(char* tb, int lane, const T* rec) {
  static_assert(sizeof(T) == 8 && C::REM2 == 0, "the shared-axes form is fp64");
#pragma unroll
  for (int c = 0; c < C::NC; ++c) {
    if (C::lin_chunk(c)) continue;
    double2 v; v.x = rec[c * 2]; v.y = rec[c * 2 + 1];
    if constexpr (NT) {
      typedef float nt4 __attribute__((ext_vector_type(4)));
      nt4 raw;
      __builtin_memcpy(&raw, &v, 16);
      __builtin_nontemporal_store(raw, reinterpret_cast<nt4*>(tb + (long)c * C::LPT * 16 + (long)lane * 16));
    } else {
      *reinterpret_cast<double2*>(tb + (long)c * C::LPT * 16 + (long)lane * 16) = v;
    }
  }
  if constexpr (C::REM1) *reinterpret_cast<T*>(tb + C::TAIL1_OFF + (long)lane * (long)sizeof(T)) = rec[C::RW - 1];
}

// QUERY: the own-time sphere-intersection query of the target (kf_aux.hpp, sphere_query) runs on the
// posterior state while it is still in registers -- BASELINE.json configs[4], "per-step interception
// point fused on-GPU": one launch per tick instead of step + query.
// PERQR: Q and R come from the target's own parameter class (a table in HBM, per-lane loads) instead of the one
// shared pair read through the scalar cache.
// Register budget the allocator must respect (wavefronts per SIMD it has to leave room for; 1 = unconstrained).  The
// per-class angular_rates kernel in fp64 on packed group blocks sits two registers over the three-wave limit (170 of 168) when
// left alone; held to it, it parks 12-24 B per lane in scratch (grouped classes 162 -> 156 us per 10^6-target tick).
// (Resident kernels are never held to a register limit that makes them spill: a kernel with scratch is also limited by the
// scratch wave slots the runtime has sized for the process, which the occupancy query does not see -- the angular_rates fp64
// kernel, 6 registers over the two-wave limit, held to it: 114 000 targets started in a fresh process and did not in one that
// had run other kernels before.)
template <class M, typename T, int LAYOUT, bool PERQR, int LIVE = 0>
constexpr int sep_min_waves() {
  // (the resident uniform-acceleration fp64 and angular-rates fp32 kernels with the per-tick query: 170 / 171 registers when
  // scheduled freely, 3 wavefronts per SIMD need 168)
  return ((PERQR && M::TYPE == ANGULAR_RATES && sizeof(T) == 8 && LAYOUT == LAYOUT_SEPARABLE_PACKED) ||
          (LIVE == 2 && M::TYPE == UNIFORM_ACCELERATION && sizeof(T) == 8) || (LIVE == 2 && M::TYPE == ANGULAR_RATES && sizeof(T) == 4)) ? 3 : 1;
}

// Resident kernels keep the whole record in registers between ticks, and the capacity of the mode is the register file.  For
// the fp64 angular models that is not enough (angular_rates: 57 words = 114 registers of state under an fp64 atan2 / asin chain
// -> 262, one wavefront per SIMD, 49 152 targets): part of the record is PARKED in the wavefront's LDS between its uses --
// every lane its own column, word-interleaved (conflict-free ds_read/write_b64), read when its chain's turn comes and written
// back behind it.  live_park_p_chains / live_park_x_chains<M, T>() = how many [p v (a)] chains park their covariance words (P) /
// their state words (x); chosen so that the resident kernels fit three wavefronts per SIMD with at most 13 KB of LDS per
// wavefront (12 per CU).  -DTE_PARK_P / -DTE_PARK_X override them for experiments (one kernel at a time through
// tools/kres.py / tools/isa_liveness.py; the library is built without them).
template <class M, typename T> constexpr int live_park_p_chains() {
#ifdef TE_PARK_P
  return TE_PARK_P;
#else
  return sizeof(T) == 8 && M::TYPE == ANGULAR_RATES ? 4 : sizeof(T) == 8 && M::TYPE == ANGULAR_VELOCITIES ? 3 : 0;
#endif
}
template <class M, typename T> constexpr int live_park_x_chains() {
#ifdef TE_PARK_X
  return TE_PARK_X;
#else
  return sizeof(T) == 8 && M::TYPE == ANGULAR_VELOCITIES ? 3 : 0;
#endif
}
template <class C, class M, typename T> struct LivePark {
  static constexpr int NLIN = M::EKF ? 3 : C::K, LB = M::EKF ? 2 : C::NB, STRIDE = M::EKF ? 6 : C::K;
  struct Table { int v[C::RW]; int count; };
  static constexpr Table make() {
    Table t{};
    for (int w = 0; w < C::RW; ++w) t.v[w] = -1;
    int k = 0;
    for (int i = 0; i < NLIN && i < live_park_p_chains<M, T>(); ++i)
      for (int b = 0; b < LB; ++b)
        for (int c = b; c < LB; ++c) t.v[C::PWORD.v[i + STRIDE * b][i + STRIDE * c]] = k++;
    for (int i = 0; i < NLIN && i < live_park_x_chains<M, T>(); ++i)
      for (int b = 0; b < LB; ++b) t.v[C::X_OFF + i + STRIDE * b] = k++;
    t.count = k;
    return t;
  }
  static constexpr Table SLOT = make();
};

// LIVE: a resident launch (StepArgs::live_*): the tick loop of FUSED with a wait for the host's doorbell in front of every tick
// and a progress word behind it (1), optionally with the per-tick sphere query and pose output (2: more registers, so fewer
// resident targets).  Same arithmetic per tick, same results as single ticks.
// AB: an A -> B tick (StepArgs::rec_out), its own instantiation (see kf_step_kernel).
// POSE: the per-tick pose stream (StepArgs::pose): after each tick, derive_outputs on the posterior still in registers, the 7
// components stored as SoA rows -- a wavefront's 64 lanes write 64 consecutive doubles per row, i.e. whole 512-byte lines.  A
// single tick writes its block behind store_record (most of P is dead by then); FUSED writes tick s's block inside the tick loop.
// INNOV: the innovation stream (StepArgs::nis): the tick's innovation nu = y - x^-[0:m] and NIS = nu^T S^-1 nu, from the values the
// update itself forms -- every chain adds nu^2 / S as it runs, axis-ascending, the EKF's attitude group adds its 3 x 3 form last --
// stored behind store_record like the pose block: lane = column, 64 consecutive doubles per row.  Without a measurement: -1 and
// zeros.  Dense single ticks in place, without the fused query or the pose output (the host adds those as launches of their own).
// The step of one wavefront's targets: `wg` = index of the wavefront among those of the launch (of the BATCH, in a population
// launch: kf_step_population_kernel below), lane = its lane.
// VAR: the variant word (step_variant.hpp), unpacked here into the names the body uses.
// GATE: the validation gate of a launched tick (StepParams::gate), with INNOV only.  The tick in two phases.  A: every chain's
// prediction and, with a measurement, its innovation, 1 / S and NIS term -- the unwrapped angles in temporaries, the unwrap
// memory untouched.  The decision: acc = has && (double)nis <= gate, so a NaN rejects.  B, under acc: the unwrap memory and every
// chain's update from the SAME 1 / S and nu.  An accepted target leaves in the bits of the plain tick with mask 1, a rejected one
// in those of the plain tick with mask 0; the stream reports NIS and nu of every measured target either way.  acc replaces the
// has-bit in everything behind it: the measurement counter (always added to nm_base) and the uniform-tile agreement (always
// tested).  `gate` is an argument of its own, not a field of StepArgs, whose size is part of every existing kernel's descriptor;
// 0 = no gate (a part of a gated population launch without one): acc = has.
// GATE with LIVE == 2 (and without INNOV): the same two-phase body inside the resident tick loop, LiveGate below.
// GATE with VAR == kFused (no live field, no INNOV): the same body and the resident policy tail inside the LAUNCHED fused tick loop,
// with the NIS rows, innovation blocks and event rows of every tick as plain stores: FusedGate below (kf_step_sep_fused_gate_kernel).
// BYID: the by-id update policy (target_manager_set_update_gate) in the gated INDEXED tick: GateById below, whose tail runs per
// valid lane behind the decision and ahead of store_record -- the slot's rejection run by target_reacquire_c's table and, on the
// K-th consecutive rejection, the record re-initialised IN REGISTERS from this entry's measurement exactly as init_kernel /
// reacquire_kernel write it (x0 = the measured pose with v0 = a0 = 0, the slot's own P0 through the layout's p_word table, unwrap
// memory 0; clock and counter untouched).  store_record, the getter-table row (o_pose) and signal_done then see the
// re-initialised state: the flush stays ONE launch.  The NIS row and the event row are indexed by ENTRY; an entry with a negative
// slot writes nothing.  An indexed launch sees settled tiles (Batch::records() settles them), so no uniform-tile code is needed
// here, in contrast to reacquire_kernel.
struct GateById {
  double gate;              // nis_max (> 0)
  int k;                    // -1: gate only (runs untouched); 0: count only; 1..127: re-initialise on the k-th consecutive rejection
  unsigned char* run;       // [slots] rejection runs (Batch::d_run_, the byte the dense calls use); unread with k < 0
  const double* p0_tab;     // [rows][N*N] initial covariances; unread with k <= 0
  const int* p0_idx;        // [slots] row of every slot
  unsigned char* event;     // [entries] this call's event bytes, or null
};

// LIVE GATE: the validation gate and the re-acquisition policy INSIDE a resident session (kf_step_sep_live_gate_kernel: VAR =
// kFused | kLive2 with GATE; target_batch_live_set_gate).  The two-phase body runs in every tick of the resident loop, and the
// policy tail behind it: no launch can follow a resident tick, so the rejection run lives in a register for the whole session
// (read from LiveGate::run at its start, written back with the records when the kernel leaves) and a lost target is
// re-initialised in registers -- and in the parked part of the record (LivePark) -- exactly as the by-id tail does it.  Tick k of
// the session (0 at its start) writes NIS row b = (nis_ring > 0 ? k % nis_ring : k) and the event row likewise: lane = column, so
// a wavefront writes 64 consecutive doubles / bytes, with system-scope stores issued ahead of the wait that precedes the tick's
// progress word -- a consumer may copy them on another stream once `done` has reached k + 1.  Nothing here waits, and every
// branch on a slot's decision is lane-predicated arithmetic and stores inside the tick: the protocol is the plain session's.
struct LiveGate {
  double gate;              // nis_max (> 0)
  double* nis;              // NIS rows of the session
  long nis_stride;          // doubles between consecutive rows (0: one row)
  long nis_ring;            // > 0: the rows form a ring
  int k;                    // -1: gate only (runs untouched); 0: count only; 1..127: re-initialise on the k-th consecutive rejection
  unsigned char* run;       // [n] rejection runs (Batch::d_run_); unread with k < 0
  const double* p0_tab;     // [rows][N*N] initial covariances; unread with k <= 0
  const int* p0_idx;        // [n] row of every slot
  unsigned char* event;     // event rows of the session, or null
  long event_stride;        // bytes between consecutive rows (0: one row)
  long event_ring;
};

// The resident kernel reads it where it arrived, in the kernel-argument segment (constant address space: scalar loads), and
// afresh in every tick: the resident loops have no scalar register to spare (they hold Q and R there), and eleven words that stay
// live across the whole loop are spilled -- which the compiler accounts as scratch, and a resident kernel must have none.
typedef const LiveGate __attribute__((address_space(4))) LiveGateArg;

// FUSED GATE: the validation gate, the innovation stream and the re-acquisition policy inside a LAUNCHED temporally fused call
// (kf_step_sep_fused_gate_kernel: VAR = kFused with GATE and without a live field; target_batch_step_fused_gated).  The resident
// kernel's loop as an ordinary launch: no relay, doorbell or progress word, a finite StepArgs::n_ticks, and nothing leaves through
// system-scope stores -- the end of the kernel orders the rows for a consumer on the stream, as for the pose stream.  Every tick
// runs the two-phase body and the policy tail; the run lives in a register from the first tick to the last (read from
// FusedGate::run ahead of the loop, written back with the records behind it) and a lost target is re-initialised in registers.
// Tick s of the call writes NIS row b = (nis_ring > 0 ? s % nis_ring : s), its innovation block b (SoA [m][innov_ld], unless innov
// is null) and its event row (its own ring): plain stores, lane = column, so a wavefront writes 64 consecutive doubles / bytes per
// row; columns >= n are never written.  gate == 0: no gate (acc = has), the plain innovation stream from a fused call.
struct FusedGate {
  double gate;              // nis_max (0: none)
  double* nis;              // NIS rows of the call
  long nis_stride;          // doubles between consecutive rows (0: one row)
  long nis_ring;            // > 0: the rows and the innovation blocks form a ring
  double* innov;            // innovation blocks [m][innov_ld] of the call, or null
  long innov_ld;
  long innov_stride;        // doubles between consecutive blocks (0: one block)
  int k;                    // -1: no policy (runs untouched); 0: count only; 1..127: re-initialise on the k-th consecutive rejection
  unsigned char* run;       // [n] rejection runs (Batch::d_run_); unread with k < 0
  const double* p0_tab;     // [rows][N*N] initial covariances; unread with k <= 0
  const int* p0_idx;        // [n] row of every slot
  unsigned char* event;     // event rows of the call, or null
  long event_stride;        // bytes between consecutive rows (0: one row)
  long event_ring;
};
// Read per tick from the kernel-argument segment, like LiveGateArg and for its reason: fourteen words held in scalar registers
// across the tick loop next to the hoisted Q and R would be spilled, and no shipped kernel has scratch.
// Both kernel arguments as they lie in the segment (explicit arguments in order, each at its natural alignment): every read is then
// a scalar load at a constant offset from the segment pointer, which a kernel holds anyway -- no second pointer to keep.
template <typename T> struct FusedGateSegment { StepArgs<T> a; FusedGate g; };
// ... and of the gated kernel with a time-step schedule (kf_step_sep_fused_gate_dt_kernel): the table's pointer is a third
// argument, read per tick from the segment like the rest
template <typename T> struct FusedGateDtSegment { StepArgs<T> a; FusedGate g; const double* dt_tab; };

// The form of the re-initialisation per instantiation.  In registers (above) where that costs no wavefront per SIMD against the
// same kernel without it; elsewhere the record is written once more BEHIND store_record, word by word through state_set /
// unwrap_ptr with the rolled loops init_kernel has, and the state words in registers are refreshed from x0 for the getter-table
// row -- still one launch.  profiles/r13_update_gate_kernel_resources.txt names the form each instantiation got.
template <class M, typename T, int LAYOUT>
constexpr bool gate_id_tail_in_registers() {
#ifdef TE_GATE_ID_TAIL
  return TE_GATE_ID_TAIL != 0;   // (experiments: one form for every instantiation, through tools/kres.py)
#else
  // the two instantiations whose register form costs a wavefront per SIMD (88 against 76 registers, 5 against 6 wavefronts; 132
  // against 128, 3 against 4); the other 18 have the same occupancy in both forms
  return !(sizeof(T) == 4 && ((M::TYPE == UNIFORM_ACCELERATION && LAYOUT == LAYOUT_SEPARABLE) ||
                              (M::TYPE == ANGULAR_VELOCITIES && LAYOUT == LAYOUT_SEPARABLE_PACKED)));
#endif
}

// DTTAB: the launched fused call with a time-step schedule (target_batch_step_fused_dt): tick s of the loop runs with dt_tab[s], a
// device table of doubles read through the constant address space like Qm -- uniform across the wavefront, one scalar load and
// one conversion per tick.  A template argument next to the variant word, as GATE is; the kernels without it compile to what they were.
// SEG: the byte offset in the kernel-argument segment at which the launched fused gated loop finds its FusedGateSegment /
// FusedGateDtSegment -- 0 for the per-batch kernels (their arguments ARE the segment), part k's element of PopulationFusedArgs::part in
// kf_step_population_fused_kernel.  A compile-time constant: every read stays a scalar load at a constant offset from the segment pointer.
template <class M, typename T, int LAYOUT, unsigned VAR, bool GATE = false, bool BYID = false, bool DTTAB = false, unsigned SEG = 0>
__device__ __forceinline__ void sep_step_wave(const StepArgs<T>& a, long wg, const int lane, const double gate = 0.0, const GateById* gid = nullptr,
                                              const LiveGateArg* lg = nullptr, const double* dt_tab = nullptr) {
  constexpr bool INDEXED = sv_has(VAR, kIndexed), FUSED = sv_has(VAR, kFused), QUERY = sv_has(VAR, kQuery), PERQR = sv_has(VAR, kPerQR),
                 AB = sv_has(VAR, kAB), POSE = sv_has(VAR, kPose), INNOV = sv_has(VAR, kInnov);
  constexpr int LIVE = sv_live(VAR);
  using C = Cfg<M, T, 1, LAYOUT>;
  static_assert(C::SEP, "separable layouts only");
  static_assert(sep_variant_ok(VAR, C::SHARED), "no such variant of the separable step (step_variant.hpp)");
  constexpr bool LGATE = GATE && LIVE != 0;   // the gate inside a resident session (LiveGate)
  constexpr bool FGATE = GATE && FUSED && LIVE == 0;   // the gate inside a launched fused call (FusedGate)
  static_assert(!GATE || INNOV || LIVE == 2 || FGATE,
                "the gate decides on the NIS of the innovation stream's kernels, inside the resident kLive2 loop, or inside the launched kFused loop");
  static_assert(!FGATE || VAR == kFused, "the launched fused gate is kFused with GATE and nothing else (its streams travel in FusedGate)");
  static_assert(BYID == (INNOV && INDEXED) && (!BYID || GATE), "kInnov | kIndexed is the gated by-id step and nothing else");
  if constexpr (!BYID) (void)gid;
  if constexpr (!LGATE) (void)lg;
  static_assert(!DTTAB || (FUSED && LIVE == 0 && !INDEXED), "the time-step table belongs to the launched fused loops");
  if constexpr (!DTTAB || FGATE) (void)dt_tab;   // (FGATE: read per tick where it arrived -- FusedGateDtSegment)
  // FGATE: the kernel's two arguments where they arrived (FusedGateSegment)
  typedef const FusedGateSegment<T> __attribute__((address_space(4))) FusedSeg;
  typedef const char __attribute__((address_space(4))) SegByte;
#define FSEG_ ((FusedSeg*)((SegByte*)__builtin_amdgcn_kernarg_segment_ptr() + SEG))
#define FG0_ (FSEG_->g)
  constexpr int N = C::N, K = C::K, NB = C::NB, TPW = C::TPW;
  using F = Mth<T>;

  if constexpr (LIVE) {   // the workgroup behind the last worker is the relay between the host's words and the device's
    const long workers = (a.n + TPW - 1) / TPW;
    if (wg == workers) {
      live_relay(a.live_posted, a.live_mirror, a.live_progress, a.live_done, workers, a.live_spin_limit, a.live_idle_ticks, lane, a.live_flags);
      return;
    }
  }
#ifdef TE_QUERY_PHASE_CLOCK
  const long long ts_begin = (long long)__builtin_readcyclecounter();
#endif
  if (wg * TPW >= a.n) return;
  const long wave_id = wg;                               // LIVE: index of this wavefront's progress word
  const long entry = wg * TPW + lane;
  bool valid = entry < a.n;
  long tile;
  int lt;
  long slot_of = entry;
  if constexpr (INDEXED) {
    long slot = valid ? (long)a.idx[entry] : -1;   // a negative slot = "skip this entry"
    valid = slot >= 0;
    if (!valid) slot = 0;
    slot_of = slot;
    tile = slot / TPW;
    lt = (int)(slot % TPW);
  } else {
    tile = wg;
    lt = lane;
  }
  char* tb = a.rec + tile * C::TILE_BYTES;
  T mem[C::RW];
  // uniform tiles: compiled into the dense launches of the shared-axes form (the indexed kernel sees settled records: Batch::settle_tiles)
  constexpr bool UT = C::UT && !INDEXED;
  int uni_flag = 0;
  bool uni = false, uni_out = false;
  constexpr bool BLK_EARLY = UT && uniform_tiles_block_early(M::TYPE);
  T blk[BLK_EARLY ? C::LW : 1];
  if constexpr (!UT) { (void)uni_flag; (void)uni; (void)uni_out; }
  if constexpr (!BLK_EARLY) (void)blk;
  // the launched dense single tick requests its measurement ahead of its record (sep_meas_first)
  constexpr bool MF = sep_meas_first<M, T, LAYOUT, VAR>();
  constexpr int MW = M::ANGULAR ? 7 : 3;
  T ymeas0[MF ? MW : 1];
  unsigned char hmask0 = 1;
  if constexpr (MF) {
#pragma unroll
    for (int c = 0; c < MW; ++c) ymeas0[c] = 0;
  } else {
    (void)ymeas0; (void)hmask0;
  }
  // LIVE: the parked part of the record (LivePark) lives in the wavefront's LDS for the whole session
  using Park = LivePark<C, M, T>;
  constexpr int NPARK = (LIVE != 0 && C::SEPPK) ? Park::SLOT.count : 0;
  __shared__ T park_lds[NPARK > 0 ? NPARK * 64 : 1];
  __shared__ double qpose_lds[LIVE == 2 ? 64 * 7 : 1];   // the per-tick query's pose rows on their way out (LIVE == 2, below)
  if constexpr (NPARK > 0) {
    // the record goes to its two homes chunk by chunk, a few loads in flight at a time: loaded whole (load_record) it would
    // itself be the register peak of the kernel.  Once per session: its speed does not matter.
    static_assert(C::REM2 == 0, "parked records: 16-byte chunks and a one-word tail");
    using V = typename Vec16<T>::type;
#pragma unroll
    for (int c = 0; c < C::NC; ++c) {
      V v{};
      if (valid) v = *reinterpret_cast<const V*>(tb + (long)c * C::LPT * 16 + (long)lt * 16);
      T w2[C::VW];
      __builtin_memcpy(w2, &v, 16);
#pragma unroll
      for (int k = 0; k < C::VW; ++k) {
        const int w = c * C::VW + k;
        if (Park::SLOT.v[w] >= 0) park_lds[Park::SLOT.v[w] * 64 + lane] = w2[k];
        else mem[w] = w2[k];
      }
      if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (C::REM1) {
      const T v = valid ? *reinterpret_cast<const T*>(tb + C::TAIL1_OFF + (long)lt * (long)sizeof(T)) : T(0);
      if (Park::SLOT.v[C::RW - 1] >= 0) park_lds[Park::SLOT.v[C::RW - 1] * 64 + lane] = v;
      else mem[C::RW - 1] = v;
    }
  } else if constexpr (MF) {
    // (sep_meas_first) The flag first: loads return in order, so waiting for it waits for nothing else.  The block of a model that
    // asks for it up front rides with the flag.
    if constexpr (UT) {
      if (a.tile_uni != nullptr) {
        uni_flag = a.tile_uni[tile];
        if constexpr (BLK_EARLY) {
#pragma unroll
          for (int k = 0; k < C::LW; ++k) blk[k] = a.tile_blk[tile * C::LW + k];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (UT) {
#pragma unroll
      for (int w = 0; w < C::RW; ++w) mem[w] = 0;
    }
    // One region for the measurement and the record: the compiler counts the loads behind the measurement words only along paths it
    // can see, and two conditions side by side would make it wait for all of them.  Every measurement word of the tick, regardless of
    // the mask, and the has-byte -- without a condition of its own, which would get a branch and a full wait: a batch without a mask
    // reads a byte of its measurement instead (the line is on its way anyhow) and ignores it.
    if (valid) {
      if (a.meas != nullptr) {   // (wave-uniform)
#pragma unroll
        for (int c = 0; c < MW; ++c) ymeas0[c] = load_meas(&a.meas[(long)c * a.meas_ld + entry], a.nt_meas);
        const unsigned char* hp = a.has_meas != nullptr ? &a.has_meas[entry] : reinterpret_cast<const unsigned char*>(&a.meas[entry]);
        hmask0 = *hp;
      }
      __builtin_amdgcn_sched_barrier(0);
      // x and the unwrap memory, then the covariance chunks that move whatever the flag says
      if constexpr (UT) load_record_part<C, T, false, kRecState>(tb, lt, mem);
      else load_record<C, T, kRecState>(tb, lt, mem);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (UT) load_record_part<C, T, false, kRecCov>(tb, lt, mem);
      else load_record<C, T, kRecCov>(tb, lt, mem);
    } else if constexpr (!UT) {
#pragma unroll
      for (int w = 0; w < C::RW; ++w) mem[w] = 0;
    }
    // behind the flag, what depends on it: the tile's block in a uniform tile, the lanes' linear-covariance chunks in another
    if constexpr (UT) {
      uni = __builtin_amdgcn_readfirstlane(uni_flag) != 0;
      if (uni) {   // (wave-uniform) every lane takes the tile's block
#pragma unroll
        for (int k = 0; k < C::LW; ++k) {
          if constexpr (BLK_EARLY) mem[C::LIN.w[k]] = blk[k];
          else mem[C::LIN.w[k]] = a.tile_blk[tile * C::LW + k];
        }
      } else if (valid) {
        load_record_part<C, T, true>(tb, lt, mem);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // every request is out: what follows waits for the words it reads, in the order they arrive
  } else if constexpr (UT) {
    // The flag first (loads return in order: waiting for it waits for nothing else), then every part of the record that moves
    // whatever the flag says.  What depends on the flag follows behind the measurement loads: the lanes' linear-covariance chunks
    // in a tile that is not uniform, the tile's block (LW words at one address for the whole wavefront) in one that is -- unless
    // the model asks for the block up front (te_layout.hpp uniform_tiles_block_early).
    if (a.tile_uni != nullptr) {
      uni_flag = a.tile_uni[tile];
      if constexpr (BLK_EARLY) {
#pragma unroll
        for (int k = 0; k < C::LW; ++k) blk[k] = a.tile_blk[tile * C::LW + k];
      }
    }
#pragma unroll
    for (int w = 0; w < C::RW; ++w) mem[w] = 0;
    if (valid) load_record_part<C, T, false>(tb, lt, mem);
  } else if (valid) {
    load_record<C, T>(tb, lt, mem);
  } else {
#pragma unroll
    for (int w = 0; w < C::RW; ++w) mem[w] = 0;
  }
  auto RD = [&](int w) -> T {
    if (NPARK > 0 && Park::SLOT.v[w] >= 0) return park_lds[Park::SLOT.v[w] * 64 + lane];
    return mem[w];
  };
  auto WR = [&](int w, T v) {
    if (NPARK > 0 && Park::SLOT.v[w] >= 0) park_lds[Park::SLOT.v[w] * 64 + lane] = v;
    else mem[w] = v;
  };
  // POSE: tick `tick`'s block of the pose stream from the state words in registers (uniform branch: a population part may have none)
  auto write_pose = [&](int tick) {
    if (a.pose == nullptr || !valid) return;
    T xq[N], pose7[7], twist6[6], acc6[6];
#pragma unroll
    for (int r = 0; r < N; ++r) xq[r] = mem[C::X_OFF + r];
    derive_outputs<M, T>(xq, false, (T)0, pose7, twist6, acc6);
    double* dst = a.pose + (a.pose_ring > 0 ? (long)tick % a.pose_ring : (long)tick) * a.pose_tick_stride + entry;
#pragma unroll
    for (int c = 0; c < 7; ++c) dst[(long)c * a.pose_ld] = (double)pose7[c];
  };
  if constexpr (!POSE) (void)write_pose;
  // INNOV: the tick's NIS row and innovation block (uniform branches: a population part may have no stream, a stream no block)
  auto write_innov = [&](bool has, T nis, const T* nu, int m) {
    if (a.nis == nullptr || !valid) return;
    a.nis[entry] = has ? (double)nis : -1.0;
    if (a.innov != nullptr) {
      for (int c = 0; c < m; ++c) a.innov[(long)c * a.innov_ld + entry] = has ? (double)nu[c] : 0.0;
    }
  };
  if constexpr (!INNOV) (void)write_innov;
  double dtd = a.dt;
  if constexpr (INDEXED) {
    if (a.dt_per && valid) dtd = a.dt_per[entry];
  }
  const T dt_call = (T)dtd;   // (DTTAB: unread -- every tick takes its own from the table)
  // The one (Q, R) row of a one-class batch, through the CONSTANT address space: uniform and never written while a step kernel
  // runs, so every read is a scalar load wherever it sits.  As a plain global pointer it stops being one behind the resident
  // loop's atomics (the compiler can no longer prove that nothing clobbers it): the fp64 angular kernels, whose 60 words do not
  // fit the scalar registers ahead of the loop, fetched them with vector loads every tick -- 120 vector registers.
  typedef const T __attribute__((address_space(4))) ConstT;
  ConstT* Qm = (ConstT*)a.qr;
  // PERQR: when every target of the wavefront belongs to ONE class -- the usual case, classes arrive in runs -- the row is
  // read through the scalar cache like the single (Q, R) of a one-class batch (Qu, a uniform address); only a wavefront
  // that mixes classes pays for per-lane gathers of its rows.
  const T* Qu = a.qr;
  bool cls_uniform = false;
  int cls_own = 0;
  if constexpr (PERQR) {
    if (valid) cls_own = a.cls[slot_of];
    const int cls_first = __builtin_amdgcn_readfirstlane(cls_own);
    cls_uniform = __all(!valid || cls_own == cls_first) != 0;   // (a ragged wave whose lane 0 is idle may take the per-lane path: same results)
    Qu = a.qr + (long)cls_first * C::QR_WORDS;
  }
  // the per-lane row, formed where it is needed (one register for the class instead of two for the address)
  auto lane_row = [&]() -> const T* {
    const T* q = a.qr + (long)cls_own * C::QR_WORDS;
    if constexpr ((C::QR_WORDS * sizeof(T)) % 16 == 0) q = static_cast<const T*>(__builtin_assume_aligned(q, 16));   // rows are whole 16-byte chunks: wide loads
    return q;
  };
  if constexpr (!PERQR) (void)lane_row;
  // the [p v (a)] chains.  Linear models: K of them, rows {i, i+K, i+2K}.  EKF: x, y, z with rows
  // {i, i+6} (position, velocity), plus the 6-state attitude group (rows 3..5, 9..11).
  constexpr int NLIN = M::EKF ? 3 : K;
  constexpr int LB = M::EKF ? 2 : NB;         // states per chain
  constexpr int STRIDE = M::EKF ? 6 : K;      // row distance between the states of a chain
  constexpr int GRA[6] = {3, 4, 5, 9, 10, 11};
  // Q and R of every chain are uniform (scalar loads): when they fit the scalar registers they are requested
  // once, here, behind the record loads, instead of chain by chain with a wait each (a serial chain of
  // scalar-cache round trips that a small, latency-bound batch feels directly).
  // Shared-axes form: axis i takes the covariance half of its chain from the first axis of its kind (`lead`); only the lead
  // chains have P words in the record and read Q and R.
  auto lead = [](int i) constexpr { return !C::SHARED || i % 3 == 0; };
  constexpr int NCOV = C::SHARED ? NLIN / 3 : NLIN;   // chains whose covariance half runs
  constexpr int QR_NEED = NCOV * LB * LB + NCOV + (M::EKF ? 36 + 9 : 0);
  // (the gated resident angular-rates fp32 kernel: its 60 hoisted words next to the gate's own push scalar registers out to
  // scratch -- 68 B, and a resident kernel must have none; it reads Q and R chain by chain instead)
  constexpr bool HOIST_QR = !PERQR && QR_NEED * (int)sizeof(T) <= 256 && !(LGATE && M::TYPE == ANGULAR_RATES && sizeof(T) == 4);
  // The launched fused gate's fp64 angular kernels read Q and R from memory every tick (480 B: not hoisted), and the compiler merges
  // the scalar loads of neighbouring chains / rows into sixteen-register requests.  In two instantiations the allocator then sets
  // up spill slots for scalar tuples -- 68 B that the compiler accounts as scratch although nothing is stored there.  Those two
  // read every chain (angular-rates on full groups) / every row of the EKF group's Q (angular-velocities on packed groups) through
  // a base pointer of its own, which keeps the requests apart; the other instantiations have no scratch as they are (and
  // angular-velocities on full groups gets 100 B WITH the separate bases).
  constexpr bool FGATE_Q_CHAIN_BASE = FGATE && sizeof(T) == 8 && M::TYPE == ANGULAR_RATES && LAYOUT == LAYOUT_SEPARABLE;
  constexpr bool FGATE_Q_ROW_BASE = FGATE && sizeof(T) == 8 && M::TYPE == ANGULAR_VELOCITIES && LAYOUT == LAYOUT_SEPARABLE_PACKED;
  T Qlin[HOIST_QR ? NLIN : 1][LB][LB], Rlin[HOIST_QR ? NLIN : 1], Qatt[HOIST_QR && M::EKF ? 6 : 1][6], Ratt[HOIST_QR && M::EKF ? 3 : 1][3];
  if constexpr (HOIST_QR) {
#pragma unroll
    for (int i = 0; i < NLIN; ++i) {
      if (!lead(i)) continue;
#pragma unroll
      for (int b = 0; b < LB; ++b)
#pragma unroll
        for (int c = 0; c < LB; ++c) Qlin[i][b][c] = Qm[C::QWORD.v[i + STRIDE * b][i + STRIDE * c]];
      Rlin[i] = Qm[C::RWORD.v[i][i]];
    }
    if constexpr (M::EKF) {
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) Qatt[r][c] = Qm[C::QWORD.v[GRA[r]][GRA[c]]];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Ratt[r][c] = Qm[C::RWORD.v[3 + r][3 + c]];
    }
  }
  // INNOV: the tick's innovations (measurement order = state rows 0..m-1) and the NIS sum (one tick per launch)
  constexpr int MI = (INNOV || LGATE || FGATE) ? (M::ANGULAR ? 6 : 3) : 1;
  T nu_all[MI], nis = T(0);
#pragma unroll
  for (int c = 0; c < MI; ++c) nu_all[c] = T(0);
  if constexpr (!INNOV && !LGATE && !FGATE) { (void)nu_all; (void)nis; }
  // GATE: what the update behind the decision takes from the prediction -- per chain 1 / S and the column P^-[1:,0] (the packed
  // records keep the upper triangle only), the unwrapped angles -- and the two masks: the tick's has-bit for the stream, acc for the rest
  constexpr int NGATE = GATE ? NCOV : 1;            // one entry per chain whose covariance half runs
  auto cov_of = [](int i) constexpr { return C::SHARED ? i / 3 : i; };
  T g_inv[NGATE], g_pcol[NGATE][LB], g_uw[3] = {0, 0, 0};
  bool g_has = false, acc = false;
  if constexpr (!GATE) { (void)g_inv; (void)g_pcol; (void)g_uw; (void)g_has; (void)acc; (void)gate; (void)cov_of; }
  // BYID, the form behind store_record: the measurement of a re-initialising lane, kept past the tick loop
  constexpr bool TAIL_REGS = !BYID || gate_id_tail_in_registers<M, T, LAYOUT>();
  T by_y[(BYID && !TAIL_REGS) ? (M::ANGULAR ? 7 : 3) : 1];
  bool by_reinit = false;
  if constexpr (!BYID || TAIL_REGS) { (void)by_y; (void)by_reinit; }
  // LGATE: the slot's rejection run, in a register for the whole session
  unsigned live_run = 0;
  long live_nis_row = 0, live_event_row = 0;   // row of the tick at hand: k, or k % ring
  if constexpr (LGATE) {
    if (lg->k >= 0 && valid) live_run = lg->run[entry];
  } else if constexpr (FGATE) {   // the same register for the launched fused call
    if (FG0_.k >= 0 && valid) live_run = FG0_.run[entry];
    (void)live_nis_row; (void)live_event_row;
  } else {
    (void)live_run; (void)live_nis_row; (void)live_event_row;
  }
  int fused_nis_row = 0, fused_event_row = 0;   // FGATE: row of the tick at hand
  if constexpr (!FGATE) { (void)fused_nis_row; (void)fused_event_row; }
  int n_has = 0;
  const int n_ticks = FUSED ? a.n_ticks : 1;
  long long live_seen = 0;
  // (FGATE: the bound read per tick as well -- FusedGateSegment)
  for (int tick = 0; tick < (FGATE ? FSEG_->a.n_ticks : n_ticks); ++tick) {
  long slot_tick = tick;
  if constexpr (LIVE) {
    // (the worker's own limit is a backstop far behind the relay's: a relay round is a PCIe read + a scan, a worker poll an L2 hit)
    if (!live_wait_tick(a.live_mirror + (wave_id / kLiveGroup) * kLiveMirrorStride, a.live_posted, (long long)tick + 1, a.live_spin_limit < 0x07000000u ? 32u * a.live_spin_limit + 10000000u : 0xffffffffu, live_seen, lane, a.live_flags)) break;
    slot_tick = (a.live_first + tick) % a.live_ring;
    if constexpr (LGATE) nis = T(0);   // (one sum per tick)
  }
  LiveGateArg* lgt = lg;   // LGATE: this tick's view of the gate's arguments (see LiveGateArg)
  if constexpr (LGATE) asm volatile("" : "+s"(lgt));
  else (void)lgt;
  // FGATE: likewise, and the tick's view of StepArgs as well (FusedGateSegment): the fp64 angular kernels spilled scalar
  // registers otherwise, which the compiler accounts as scratch
  // (SEG is added behind the barrier: it then folds into every load's constant offset instead of costing scalar address arithmetic per tick)
  SegByte* kt0 = FGATE ? (SegByte*)__builtin_amdgcn_kernarg_segment_ptr() : nullptr;
  if constexpr (FGATE) {
    asm volatile("" : "+s"(kt0));
    nis = T(0);   // (one sum per tick)
  }
  FusedSeg* kt = (FusedSeg*)(kt0 + (FGATE ? SEG : 0u));
  (void)kt;
  const auto* const fgt = &kt->g;
  const auto* const at = &kt->a;
  (void)fgt; (void)at;
  // the tick's dt: the launch's, or (DTTAB) entry `tick` of the schedule -- a scalar load at a uniform address, converted once
  T dt_tick = dt_call;
  if constexpr (DTTAB) {
    // base + a 32-bit byte offset: the scalar load's own addressing form, no 64-bit address arithmetic in scalar registers (with it
    // the gated angular-velocities fp64 kernel on packed groups had 36 B of scalar spill slots accounted as scratch).  The host
    // launches at most kDtTabMaxTicks ticks (dt_schedule.hpp) with a table -- Batch::step_fused_gated runs a longer call as single
    // ticks -- so the offset cannot wrap.
    typedef const double __attribute__((address_space(4))) ConstD;
    typedef const char __attribute__((address_space(4))) ConstB;
    typedef const FusedGateDtSegment<T> __attribute__((address_space(4))) FusedDtSeg;
    const unsigned dt_off = (unsigned)tick << 3;
    if constexpr (FGATE) dt_tick = (T) * (ConstD*)((ConstB*)((FusedDtSeg*)kt)->dt_tab + dt_off);
    else dt_tick = (T) * (ConstD*)((ConstB*)dt_tab + dt_off);
  }
  const T dt = dt_tick;
#define GATE_T_ (LGATE ? lgt->gate : FGATE ? fgt->gate : gate)
  // the policy's arguments of a gate that lives inside a tick loop (constant condition: only the live arm is compiled)
#define PG_(f_) (LGATE ? lgt->f_ : fgt->f_)
#define A_(f_) (FGATE ? at->f_ : a.f_)
  const T* meas_t = A_(meas) ? A_(meas) + slot_tick * A_(tick_stride) : nullptr;
  const unsigned char* has_t = A_(has_meas) ? A_(has_meas) + slot_tick * A_(has_stride) : nullptr;
  // Every measurement word of the tick is requested up front, right behind the record loads and regardless
  // of the mask: with a cache-resident state they are the only operands that come from HBM itself, and one
  // round trip for all of them replaces one per axis.
  // (MF: they were, ahead of the record -- the one tick of the launch)
  T ymeas[MW];
#pragma unroll
  for (int c = 0; c < MW; ++c) ymeas[c] = 0;
  unsigned char hmask = 1;
  if constexpr (MF) {
#pragma unroll
    for (int c = 0; c < MW; ++c) ymeas[c] = ymeas0[c];
    // the byte is looked at here, behind every request, and not where it was asked for: left to itself the compiler forms
    // `byte != 0` next to the load and waits for the measurement there, ahead of the record's requests
    unsigned hraw = hmask0;
    asm volatile("" : "+v"(hraw));
    hmask = has_t != nullptr ? (unsigned char)hraw : (unsigned char)1;   // (without a mask the byte read was a stand-in)
  } else if (valid && meas_t != nullptr) {
#pragma unroll
    for (int c = 0; c < MW; ++c) {
      if constexpr (LIVE) ymeas[c] = load_meas_live(&meas_t[(long)c * a.meas_ld + entry]);   // (no per-load run-time choice here: it would get a branch and a wait per word)
      else ymeas[c] = load_meas(&meas_t[(long)c * A_(meas_ld) + entry], A_(nt_meas));
    }
    if (has_t != nullptr) {
      if constexpr (LIVE) hmask = (unsigned char)__hip_atomic_load(&has_t[entry], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else hmask = has_t[entry];
    }
  }
  const bool has = valid && meas_t != nullptr && hmask != 0;
  if constexpr (!GATE) n_has += has ? 1 : 0;
  if constexpr (UT && !MF) {
    uni = __builtin_amdgcn_readfirstlane(uni_flag) != 0;
    if (uni) {   // (wave-uniform) every lane takes the tile's block
#pragma unroll
      for (int k = 0; k < C::LW; ++k) {
        if constexpr (BLK_EARLY) mem[C::LIN.w[k]] = blk[k];
        else mem[C::LIN.w[k]] = a.tile_blk[tile * C::LW + k];
      }
    } else if (valid) {
      load_record_part<C, T, true>(tb, lt, mem);
    }
  }
  if constexpr (HOIST_QR) {
    // pin the hoisted Q / R values into scalar registers here, i.e. wait for their loads now, while the record
    // and measurement loads are still in flight (otherwise the compiler sinks them back next to their uses)
    if (tick == 0) {
#pragma unroll
      for (int i = 0; i < NLIN; ++i) {
        if (!lead(i)) continue;
#pragma unroll
        for (int b = 0; b < LB; ++b)
#pragma unroll
          for (int c = 0; c < LB; ++c) asm volatile("" : "+s"(Qlin[i][b][c]));
        asm volatile("" : "+s"(Rlin[i]));
      }
      if constexpr (M::EKF) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) asm volatile("" : "+s"(Qatt[r][c]));
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) asm volatile("" : "+s"(Ratt[r][c]));
      }
    }
  }

  T mrpy[3] = {0, 0, 0};
  if constexpr (M::ANGULAR) {
    if (has) {
      T q[4];
      q[0] = ymeas[3];
      q[1] = ymeas[4];
      q[2] = ymeas[5];
      q[3] = ymeas[6];
      quat_normalize(q);
      quat_to_rpy<T, (LIVE != 0 && sizeof(T) == 8)>(q, mrpy);
    }
    // MF: the conversion has waited for the measurement alone; nothing that reads the record moves up into it
    if constexpr (MF) __builtin_amdgcn_sched_barrier(0);
  }
#define XW_(r) mem[C::X_OFF + (r)]
  // the GATE body's words: a register, or in a resident session (NPARK > 0) possibly a parked word.  Macros with the constant test
  // in front, not RD / WR: the launched gated kernels must compile to what they were
#define GR_(w_) (((NPARK > 0) && Park::SLOT.v[(w_)] >= 0) ? park_lds[Park::SLOT.v[(w_)] * 64 + lane] : mem[(w_)])
#define GW_(w_, val_) do { if ((NPARK > 0) && Park::SLOT.v[(w_)] >= 0) park_lds[Park::SLOT.v[(w_)] * 64 + lane] = (val_); else mem[(w_)] = (val_); } while (0)
#define UWW_(s) mem[C::UW_OFF + (s)]
#define XR_(r) RD(C::X_OFF + (r))
#define XS_(r, v) WR(C::X_OFF + (r), (v))

  // EKF group: the Jacobians of the transition at the previous posterior read the group's x words alone (roll, pitch and the body
  // rates wy, wz, which no [p v] chain writes).  MF: formed here, behind the measurement's conversion and ahead of the first use of a
  // P word, i.e. while the covariance chunks are still on their way; otherwise where the group's turn comes.  One text for both places.
  // geometry.hpp:394-426 (Jacobians at the previous posterior), :359-374 (EarBaseInv)
#define TE_EKF_JACOBIAN_(Jr, Jw, Ei, roll_, pitch_, wy_, wz_)                                      \
  do {                                                                                              \
    T s_r, c_r, s_p, c_p;                                                                           \
    F::sincos(roll_, &s_r, &c_r);                                                                   \
    F::sincos(pitch_, &s_p, &c_p);                                                                  \
    const T wy = wy_, wz = wz_;                                                                     \
    Jr[0][0] = (dt * (wy * c_r * s_p - wz * s_p * s_r)) / c_p + 1;                                  \
    Jr[0][1] = (dt * (wz * c_r + wy * s_r)) / (c_p * c_p);                                          \
    Jr[0][2] = 0;                                                                                   \
    Jr[1][0] = -dt * (wz * c_r + wy * s_r);                                                         \
    Jr[1][1] = 1;                                                                                   \
    Jr[1][2] = 0;                                                                                   \
    Jr[2][0] = (dt * (wy * c_r - wz * s_r)) / c_p;                                                  \
    Jr[2][1] = (dt * s_p * (wz * c_r + wy * s_r)) / (c_p * c_p);                                    \
    Jr[2][2] = 1;                                                                                   \
    Jw[0][0] = dt; Jw[0][1] = (dt * s_p * s_r) / c_p; Jw[0][2] = (dt * c_r * s_p) / c_p;            \
    Jw[1][0] = 0;  Jw[1][1] = dt * c_r;               Jw[1][2] = -dt * s_r;                         \
    Jw[2][0] = 0;  Jw[2][1] = (dt * s_r) / c_p;       Jw[2][2] = (dt * c_r) / c_p;                  \
    Ei[0][0] = 1; Ei[0][1] = (s_p * s_r) / c_p; Ei[0][2] = (c_r * s_p) / c_p;                       \
    Ei[1][0] = 0; Ei[1][1] = c_r;               Ei[1][2] = -s_r;                                    \
    Ei[2][0] = 0; Ei[2][1] = s_r / c_p;         Ei[2][2] = c_r / c_p;                               \
  } while (0)
  constexpr bool JAC_EARLY = MF && M::EKF;
  T Jr0[JAC_EARLY ? 3 : 1][3], Jw0[JAC_EARLY ? 3 : 1][3], Ei0[JAC_EARLY ? 3 : 1][3];
  if constexpr (JAC_EARLY) {
    TE_EKF_JACOBIAN_(Jr0, Jw0, Ei0, XW_(3), XW_(4), XW_(10), XW_(11));
    __builtin_amdgcn_sched_barrier(0);
  } else {
    (void)Jr0; (void)Jw0; (void)Ei0;
  }

  // ---- the [p v (a)] chains
  if constexpr (GATE) {
    // phase A (sep_gate_predict_*): every chain's prediction into the record's words; with a measurement, nu, 1 / S, the NIS term
    g_has = has;
#pragma unroll
    for (int i = 0; i < NLIN; ++i) {
      const int ic = cov_of(i);   // the covariance chain this axis takes its 1 / S from
      if (lead(i)) {   // (a constant once the loop is unrolled)
        T Pb[LB][LB], Qb[LB][LB];
        ConstT* Qc = Qm;   // (FGATE_Q_CHAIN_BASE: a base of its own per chain)
        if constexpr (FGATE_Q_CHAIN_BASE) asm volatile("" : "+s"(Qc));
#pragma unroll
        for (int b = 0; b < LB; ++b)
#pragma unroll
          for (int c = 0; c < LB; ++c) {
            Pb[b][c] = GR_(C::PWORD.v[i + STRIDE * b][i + STRIDE * c]);   // (GR_ / GW_: a parked word in a resident session)
            if constexpr (HOIST_QR) Qb[b][c] = Qlin[i][b][c];
            else Qb[b][c] = Qc[C::QWORD.v[i + STRIDE * b][i + STRIDE * c]];
          }
        T r_meas;
        if constexpr (HOIST_QR) r_meas = Rlin[i];
        else r_meas = Qc[C::RWORD.v[i][i]];
        sep_gate_predict_P<LB, T>(Pb, Qb, dt);
        g_inv[ic] = T(0);
        if (has) g_inv[ic] = (T)1 / (Pb[0][0] + r_meas);
#pragma unroll
        for (int b = 0; b < LB; ++b) {
          g_pcol[ic][b] = Pb[b][0];
#pragma unroll
          for (int c = ((C::SEPPK || C::SHARED) ? b : 0); c < LB; ++c) GW_(C::PWORD.v[i + STRIDE * b][i + STRIDE * c], Pb[b][c]);
        }
      }
      T xs[LB];
#pragma unroll
      for (int b = 0; b < LB; ++b) xs[b] = GR_(C::X_OFF + i + STRIDE * b);
      T y = 0;
      if (has) {
        if (!M::ANGULAR || i < 3) {
          y = ymeas[i];
        } else {
          y = unwrap_angle(UWW_(i - 3), mrpy[i - 3]);   // angular_rates.cpp:85-88; stored in phase B
          g_uw[i - 3] = y;
        }
      }
      sep_gate_predict_x<LB, T>(xs, dt);
      {
#pragma clang fp contract(off)
        if (has) {
          nu_all[i] = y - xs[0];
          nis = nis + (nu_all[i] * nu_all[i]) * g_inv[ic];
        }
      }
#pragma unroll
      for (int b = 0; b < LB; ++b) GW_(C::X_OFF + i + STRIDE * b, xs[b]);
      if constexpr (NPARK > 0) __builtin_amdgcn_sched_barrier(0);   // a parked chain's words are read when its turn comes, not ahead of it
    }
  } else if constexpr (C::SHARED) {
    // one covariance half per kind of axis (its lead axis i % 3 == 0 owns the kind's block), one state half per axis
    T Kg[LB];
    T inv_kind = T(0);   // (INNOV) 1 / S of the kind of axis, from its lead axis
    if constexpr (!INNOV) (void)inv_kind;
#pragma unroll
    for (int b = 0; b < LB; ++b) Kg[b] = T(0);
#pragma unroll
    for (int i = 0; i < NLIN; ++i) {
      if (lead(i)) {   // (a constant once the loop is unrolled)
        T Pb[LB][LB], Qb[LB][LB];
#pragma unroll
        for (int b = 0; b < LB; ++b)
#pragma unroll
          for (int c = 0; c < LB; ++c) {
            Pb[b][c] = mem[C::PWORD.v[i + STRIDE * b][i + STRIDE * c]];
            if constexpr (HOIST_QR) Qb[b][c] = Qlin[i][b][c];
            else Qb[b][c] = Qm[C::QWORD.v[i + STRIDE * b][i + STRIDE * c]];
          }
        T r_meas;
        if constexpr (HOIST_QR) r_meas = Rlin[i];
        else r_meas = Qm[C::RWORD.v[i][i]];
        sep_linear_cov<LB, T, INNOV>(Pb, Qb, r_meas, dt, has, Kg, &inv_kind);
#pragma unroll
        for (int b = 0; b < LB; ++b)
#pragma unroll
          for (int c = b; c < LB; ++c) mem[C::PWORD.v[i + STRIDE * b][i + STRIDE * c]] = Pb[b][c];
      }
      T xs[LB];
#pragma unroll
      for (int b = 0; b < LB; ++b) xs[b] = XW_(i + STRIDE * b);
      T y = 0;
      if (has) {
        if (!M::ANGULAR || i < 3) {
          y = ymeas[i];
        } else {
          y = unwrap_angle(UWW_(i - 3), mrpy[i - 3]);   // angular_rates.cpp:85-88
          UWW_(i - 3) = y;
        }
      }
      sep_linear_state<LB, T, INNOV>(xs, dt, has, y, Kg, &nu_all[INNOV ? i : 0]);
      if constexpr (INNOV) {
#pragma clang fp contract(off)
        if (has) nis = nis + (nu_all[i] * nu_all[i]) * inv_kind;
      }
#pragma unroll
      for (int b = 0; b < LB; ++b) XW_(i + STRIDE * b) = xs[b];
    }
  } else {
#pragma unroll
    for (int i = 0; i < NLIN; ++i) {
      T xs[LB], Pb[LB][LB], Qb[LB][LB];
      T r_meas = T(0);   // (every path assigns it; the per-class branches hide that from the compiler)
#pragma unroll
      for (int b = 0; b < LB; ++b) {
        xs[b] = XR_(i + STRIDE * b);
#pragma unroll
        for (int c = 0; c < LB; ++c) Pb[b][c] = RD(C::PWORD.v[i + STRIDE * b][i + STRIDE * c]);
      }
      if constexpr (HOIST_QR) {
#pragma unroll
        for (int b = 0; b < LB; ++b)
#pragma unroll
          for (int c = 0; c < LB; ++c) Qb[b][c] = Qlin[i][b][c];
        r_meas = Rlin[i];
      } else {
        if constexpr (PERQR) {
          const T* Qsrc = lane_row();
          if (cls_uniform) {   // wave-uniform branch: scalar loads from the one row
#pragma unroll
            for (int b = 0; b < LB; ++b)
#pragma unroll
              for (int c = 0; c < LB; ++c) Qb[b][c] = Qu[C::QWORD.v[i + STRIDE * b][i + STRIDE * c]];
            r_meas = Qu[C::RWORD.v[i][i]];
            Qsrc = nullptr;
          }
          if (Qsrc != nullptr) {
#pragma unroll
            for (int b = 0; b < LB; ++b)
#pragma unroll
              for (int c = 0; c < LB; ++c) Qb[b][c] = Qsrc[C::QWORD.v[i + STRIDE * b][i + STRIDE * c]];
            r_meas = Qsrc[C::RWORD.v[i][i]];
          }
        } else {
#pragma unroll
          for (int b = 0; b < LB; ++b)
#pragma unroll
            for (int c = 0; c < LB; ++c) Qb[b][c] = Qm[C::QWORD.v[i + STRIDE * b][i + STRIDE * c]];
          r_meas = Qm[C::RWORD.v[i][i]];
        }
      }
      T y = 0;
      if (has) {
        if (!M::ANGULAR || i < 3) {
          y = ymeas[i];
        } else {
          y = unwrap_angle(UWW_(i - 3), mrpy[i - 3]);   // angular_rates.cpp:85-88
          UWW_(i - 3) = y;
        }
      }
      if constexpr (INNOV) {
#pragma clang fp contract(off)
        T inv_i = T(0);
        sep_linear_axis<LB, T, true>(xs, Pb, Qb, r_meas, dt, has, y, &inv_i, &nu_all[i]);
        if (has) nis = nis + (nu_all[i] * nu_all[i]) * inv_i;
      } else {
        sep_linear_axis<LB, T>(xs, Pb, Qb, r_meas, dt, has, y);
      }
#pragma unroll
      for (int b = 0; b < LB; ++b) {
        XS_(i + STRIDE * b, xs[b]);
#pragma unroll
        for (int c = (C::SEPPK ? b : 0); c < LB; ++c) WR(C::PWORD.v[i + STRIDE * b][i + STRIDE * c], Pb[b][c]);
      }
      if constexpr (NPARK > 0) __builtin_amdgcn_sched_barrier(0);   // a parked chain's words are read when its turn comes, not ahead of it
    }
  }

  // ---- EKF attitude group: local rows 0..2 = rpy (global 3..5), 3..5 = omega (global 9..11)
  if constexpr (M::EKF) {
    constexpr int GR[6] = {3, 4, 5, 9, 10, 11};
    T xr[6], Pr[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      xr[r] = XW_(GR[r]);
#pragma unroll
      for (int c = 0; c < 6; ++c) Pr[r][c] = mem[C::PWORD.v[GR[r]][GR[c]]];
    }
    T Jr[3][3], Jw[3][3], Ei[3][3];
    if constexpr (JAC_EARLY) {   // formed ahead of the chains, under the P loads
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) { Jr[r][c] = Jr0[r][c]; Jw[r][c] = Jw0[r][c]; Ei[r][c] = Ei0[r][c]; }
    } else {
      TE_EKF_JACOBIAN_(Jr, Jw, Ei, xr[0], xr[1], xr[4], xr[5]);
    }
    // x^- = f(x): rpy += dt * EarBaseInv(rpy) * omega  (angular_velocities.cpp:137)
    {
      T nr[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        T acc = (dt * Ei[c][0]) * xr[3];
        acc = F::fma(dt * Ei[c][1], xr[4], acc);
        acc = F::fma(dt * Ei[c][2], xr[5], acc);
        nr[c] = xr[c] + acc;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) xr[c] = nr[c];
    }
    // A P: rows 0..2 = Jr P[0:3,:] + Jw P[3:6,:]; rows 3..5 unchanged
    {
      T np[3][6];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          T v = Jr[r][0] * Pr[0][c];
          v = F::fma(Jr[r][1], Pr[1][c], v);
          v = F::fma(Jr[r][2], Pr[2][c], v);
          v = F::fma(Jw[r][0], Pr[3][c], v);
          v = F::fma(Jw[r][1], Pr[4][c], v);
          v = F::fma(Jw[r][2], Pr[5][c], v);
          np[r][c] = v;
        }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) Pr[r][c] = np[r][c];
    }
    // (A P) A^T: columns 0..2, then + Q
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      T nw[3];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        T v = Pr[r][0] * Jr[cc][0];
        v = F::fma(Pr[r][1], Jr[cc][1], v);
        v = F::fma(Pr[r][2], Jr[cc][2], v);
        v = F::fma(Pr[r][3], Jw[cc][0], v);
        v = F::fma(Pr[r][4], Jw[cc][1], v);
        v = F::fma(Pr[r][5], Jw[cc][2], v);
        nw[cc] = v;
      }
      T qrow[6];
      if constexpr (HOIST_QR) {
#pragma unroll
        for (int c = 0; c < 6; ++c) qrow[c] = Qatt[r][c];
      } else {
        if constexpr (PERQR) {
          if (cls_uniform) {
#pragma unroll
            for (int c = 0; c < 6; ++c) qrow[c] = Qu[C::QWORD.v[GR[r]][GR[c]]];
          } else {
            const T* Qsrc = lane_row();
#pragma unroll
            for (int c = 0; c < 6; ++c) qrow[c] = Qsrc[C::QWORD.v[GR[r]][GR[c]]];
          }
        } else if constexpr (FGATE_Q_ROW_BASE) {
          ConstT* Qr = Qm;   // (a base of its own per row: see FGATE_Q_ROW_BASE)
          asm volatile("" : "+s"(Qr));
#pragma unroll
          for (int c = 0; c < 6; ++c) qrow[c] = Qr[C::QWORD.v[GR[r]][GR[c]]];
        } else {
#pragma unroll
          for (int c = 0; c < 6; ++c) qrow[c] = Qm[C::QWORD.v[GR[r]][GR[c]]];
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) Pr[r][c] = (c < 3 ? nw[c < 3 ? c : 0] : Pr[r][c]) + qrow[c];
    }
    if constexpr (GATE) {
      // phase A of the group: S, its inverse, nu and the NIS term; the decision (the group is the last term of the sum); phase B
      T S[3][3], nu[3] = {0, 0, 0};
      if (has) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            T rrc;
            if constexpr (HOIST_QR) rrc = Ratt[r][c];
            else rrc = Qm[C::RWORD.v[3 + r][3 + c]];
            S[r][c] = Pr[r][c] + rrc;
          }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const T inv = (T)1 / S[p][p];
          S[p][p] = 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) S[p][c] *= inv;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            if (r == p) continue;
            const T f = S[r][p];
            S[r][p] = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) S[r][c] = F::fma(-f, S[p][c], S[r][c]);
          }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const T y = unwrap_angle(UWW_(c), mrpy[c]);   // angular_velocities.cpp:93-96; stored under acc
          g_uw[c] = y;
          nu[c] = y - xr[c];
        }
        {
#pragma clang fp contract(off)
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            nu_all[3 + r] = nu[r];
            T w = S[r][0] * nu[0];
            w = F::fma(S[r][1], nu[1], w);
            w = F::fma(S[r][2], nu[2], w);
            nis = F::fma(nu[r], w, nis);
          }
        }
      }
      acc = has && (GATE_T_ == 0.0 || (double)nis <= GATE_T_);
      if (acc) {
#pragma unroll
        for (int c = 0; c < 3; ++c) UWW_(c) = g_uw[c];
        T Kg[6][3];
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) Kg[r][l] = (c == 0) ? Pr[r][0] * S[0][l] : F::fma(Pr[r][c], S[c][l], Kg[r][l]);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          T ac = Kg[r][0] * nu[0];
          ac = F::fma(Kg[r][1], nu[1], ac);
          ac = F::fma(Kg[r][2], nu[2], ac);
          xr[r] += ac;
        }
        T D[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int j = 0; j < 3; ++j) D[r][j] = ((r == j) ? (T)1 : (T)0) - Kg[r][j];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const T t0 = Pr[0][c], t1 = Pr[1][c], t2 = Pr[2][c];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            T ac = D[r][0] * t0;
            ac = F::fma(D[r][1], t1, ac);
            ac = F::fma(D[r][2], t2, ac);
            Pr[r][c] = (r < 3) ? ac : ac + Pr[r][c];
          }
        }
      }
    } else if (has) {
      T S[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          T rrc;
          if constexpr (HOIST_QR) rrc = Ratt[r][c];
          else if constexpr (PERQR) rrc = cls_uniform ? Qu[C::RWORD.v[3 + r][3 + c]] : lane_row()[C::RWORD.v[3 + r][3 + c]];
          else rrc = Qm[C::RWORD.v[3 + r][3 + c]];
          S[r][c] = Pr[r][c] + rrc;
        }
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const T inv = (T)1 / S[p][p];
        S[p][p] = 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) S[p][c] *= inv;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          if (r == p) continue;
          const T f = S[r][p];
          S[r][p] = 0;
#pragma unroll
          for (int c = 0; c < 3; ++c) S[r][c] = F::fma(-f, S[p][c], S[r][c]);
        }
      }
      T nu[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const T y = unwrap_angle(UWW_(c), mrpy[c]);   // angular_velocities.cpp:93-96
        UWW_(c) = y;
        nu[c] = y - xr[c];
      }
      if constexpr (INNOV) {   // the attitude group's term, last: sum_r sum_c nu_r S^-1[r][c] nu_c with the inverse the gain uses
#pragma clang fp contract(off)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          nu_all[3 + r] = nu[r];
          T w = S[r][0] * nu[0];
          w = F::fma(S[r][1], nu[1], w);
          w = F::fma(S[r][2], nu[2], w);
          nis = F::fma(nu[r], w, nis);
        }
      }
      T Kg[6][3];
#pragma unroll
      for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int r = 0; r < 6; ++r) Kg[r][l] = (c == 0) ? Pr[r][0] * S[0][l] : F::fma(Pr[r][c], S[c][l], Kg[r][l]);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        T acc = Kg[r][0] * nu[0];
        acc = F::fma(Kg[r][1], nu[1], acc);
        acc = F::fma(Kg[r][2], nu[2], acc);
        xr[r] += acc;
      }
      T D[6][3];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) D[r][j] = ((r == j) ? (T)1 : (T)0) - Kg[r][j];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const T t0 = Pr[0][c], t1 = Pr[1][c], t2 = Pr[2][c];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          T acc = D[r][0] * t0;
          acc = F::fma(D[r][1], t1, acc);
          acc = F::fma(D[r][2], t2, acc);
          Pr[r][c] = (r < 3) ? acc : acc + Pr[r][c];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      XW_(GR[r]) = xr[r];
#pragma unroll
      for (int c = (C::SEPPK ? r : 0); c < 6; ++c) mem[C::PWORD.v[GR[r]][GR[c]]] = Pr[r][c];
    }
  }

  if constexpr (GATE) {
    if constexpr (!M::EKF) acc = has && (GATE_T_ == 0.0 || (double)nis <= GATE_T_);
    n_has += acc ? 1 : 0;
    // phase B: the unwrap memory and every chain's update, from the 1 / S, P^-[:,0] and nu of phase A.  As in the shared form's
    // plain loop, a lead axis forms the gain and runs the covariance half; every axis runs its state half with that gain.
    if (acc) {
      if constexpr (M::ANGULAR && !M::EKF) {
#pragma unroll
        for (int c = 0; c < 3; ++c) UWW_(c) = g_uw[c];
      }
      T Kg[LB];
#pragma unroll
      for (int b = 0; b < LB; ++b) Kg[b] = T(0);
#pragma unroll
      for (int i = 0; i < NLIN; ++i) {
        if (lead(i)) {   // (a constant once the loop is unrolled; every axis outside the shared form)
          const int ic = cov_of(i);
          sep_gate_gain<LB, T>(g_pcol[ic], g_inv[ic], Kg);
          T Pb[LB][LB];
#pragma unroll
          for (int b = 0; b < LB; ++b)
#pragma unroll
            for (int c = 0; c < LB; ++c) Pb[b][c] = (c == 0) ? g_pcol[ic][b] : GR_(C::PWORD.v[i + STRIDE * b][i + STRIDE * c]);
          sep_gate_update_P<LB, T>(Pb, Kg);
#pragma unroll
          for (int b = 0; b < LB; ++b)
#pragma unroll
            for (int c = ((C::SEPPK || C::SHARED) ? b : 0); c < LB; ++c) GW_(C::PWORD.v[i + STRIDE * b][i + STRIDE * c], Pb[b][c]);
        }
        T xs[LB];
#pragma unroll
        for (int b = 0; b < LB; ++b) xs[b] = GR_(C::X_OFF + i + STRIDE * b);
        sep_gate_update_x<LB, T>(xs, Kg, nu_all[i]);
#pragma unroll
        for (int b = 0; b < LB; ++b) GW_(C::X_OFF + i + STRIDE * b, xs[b]);
        if constexpr (NPARK > 0) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  if constexpr (LGATE || FGATE) {
    // the policy tail of the resident tick (LiveGate) and of a tick of the launched fused call (FusedGate): the run in its register,
    // the event byte and -- rarely -- the record's words replaced where they live, registers and parked words alike; then the tick's
    // NIS and event rows (FGATE: and its innovation block), lane = column
    unsigned char ev = 0;
    if (PG_(k) >= 0 && g_has) {   // (g_has: a valid lane with a measurement)
      unsigned run = 0;
      if (!acc) {   // rejected (a NaN rejects)
        const unsigned c1 = live_run + 1 < 127u ? live_run + 1 : 127u;
        ev = (unsigned char)c1; run = c1;
        if (PG_(k) > 0 && c1 >= (unsigned)PG_(k)) {   // a candidate: x0 as init_kernel forms it, re-initialised iff finite
          T x0[N];
#pragma unroll
          for (int r = 0; r < N; ++r) x0[r] = 0;
          if constexpr (M::ANGULAR) {
            T p6[6];
            pose7_to_pose6(ymeas, p6);
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) x0[c6] = p6[c6];
          } else {
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) x0[c3] = ymeas[c3];
          }
          bool reinit = true;
#pragma unroll
          for (int r = 0; r < K; ++r) reinit = reinit && (x0[r] - x0[r] == (T)0);   // finite
          if (reinit) {
            ev = (unsigned char)(0x80u | c1); run = 0;
            const double* P0 = PG_(p0_tab) + (long)PG_(p0_idx)[entry] * N * N;
#pragma unroll
            for (int r = 0; r < N; ++r) {
              XS_(r, x0[r]);
#pragma unroll
              for (int c = (C::SEPPK ? r : 0); c < N; ++c)
                if (C::PWORD.v[r][c] >= 0) WR(C::PWORD.v[r][c], (T)P0[r * N + c]);   // (state_set's words, in its order)
            }
            if constexpr (M::ANGULAR) {
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) UWW_(cc) = 0;
            }
          }
        }
      }
      live_run = run;
    }
    if constexpr (LGATE) {
      if (valid) {
        double* const nrow = lgt->nis + live_nis_row * lgt->nis_stride;
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(&nrow[entry]), (unsigned long long)__double_as_longlong(g_has ? (double)nis : -1.0),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (lgt->event != nullptr) {
          unsigned char* const erow = lgt->event + live_event_row * lgt->event_stride;
          __hip_atomic_store(&erow[entry], ev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
      // the rows of the next tick: counted, not divided (k % ring of two 64-bit words costs the scalar registers a tick has none to spare of)
      live_nis_row = live_nis_row + 1 == lgt->nis_ring ? 0 : live_nis_row + 1;
      live_event_row = live_event_row + 1 == lgt->event_ring ? 0 : live_event_row + 1;
    } else {
      if (valid) {   // plain stores: the end of the kernel orders them for a consumer on the stream
        fgt->nis[(long)fused_nis_row * fgt->nis_stride + entry] = g_has ? (double)nis : -1.0;
        if (fgt->innov != nullptr) {
          double* const nublk = fgt->innov + (long)fused_nis_row * fgt->innov_stride + entry;
#pragma unroll
          for (int c = 0; c < MI; ++c) nublk[(long)c * fgt->innov_ld] = g_has ? (double)nu_all[c] : 0.0;
        }
        if (fgt->event != nullptr) fgt->event[(long)fused_event_row * fgt->event_stride + entry] = ev;
      }
      // (n_ticks is an int, so the rows are: one scalar register each)
      fused_nis_row = (long)fused_nis_row + 1 == fgt->nis_ring ? 0 : fused_nis_row + 1;
      fused_event_row = (long)fused_event_row + 1 == fgt->event_ring ? 0 : fused_event_row + 1;
    }
  }
  if constexpr (BYID) {
    // the policy tail (GateById): run, event byte and -- rarely -- the record's words replaced in registers
    unsigned char ev = 0;
    if (gid->k >= 0 && g_has) {   // (g_has: a valid lane with a measurement)
      unsigned char* const runp = gid->run + slot_of;
      unsigned run = 0;
      if (!acc) {   // rejected (a NaN rejects)
        const unsigned c0 = *runp;
        const unsigned c1 = c0 + 1 < 127u ? c0 + 1 : 127u;
        ev = (unsigned char)c1; run = c1;
        if (gid->k > 0 && c1 >= (unsigned)gid->k) {   // a candidate: x0 as init_kernel forms it, re-initialised iff finite
          T x0[N];
#pragma unroll
          for (int r = 0; r < N; ++r) x0[r] = 0;
          if constexpr (M::ANGULAR) {
            T p6[6];
            pose7_to_pose6(ymeas, p6);
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) x0[c6] = p6[c6];
          } else {
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) x0[c3] = ymeas[c3];
          }
          bool reinit = true;
#pragma unroll
          for (int r = 0; r < K; ++r) reinit = reinit && (x0[r] - x0[r] == (T)0);   // finite
          if (reinit) { ev = (unsigned char)(0x80u | c1); run = 0; }
          if constexpr (!TAIL_REGS) {
            by_reinit = reinit;
#pragma unroll
            for (int c7 = 0; c7 < (M::ANGULAR ? 7 : 3); ++c7) by_y[c7] = ymeas[c7];
          } else if (reinit) {
            const double* P0 = gid->p0_tab + (long)gid->p0_idx[slot_of] * N * N;
#pragma unroll
            for (int r = 0; r < N; ++r) {
              XW_(r) = x0[r];
#pragma unroll
              for (int c = (C::SEPPK ? r : 0); c < N; ++c)
                if (C::PWORD.v[r][c] >= 0) mem[C::PWORD.v[r][c]] = (T)P0[r * N + c];   // (state_set's words, in its order)
            }
            if constexpr (M::ANGULAR) {
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) UWW_(cc) = 0;
            }
          }
        }
      }
      *runp = (unsigned char)run;
    }
    if (valid && gid->event != nullptr) gid->event[entry] = ev;
  }
  if constexpr (LIVE == 2) {
    // the own-time sphere query of every target after every tick (BASELINE configs[4]), on the posterior still in registers,
    // and / or the tick's poses for a consumer outside the kernel.  Run-time choices inside the LIVE == 2 variant only: the
    // query's fp64 quartic and the pose derivation cost 30 - 60 registers, i.e. resident capacity, which a plain session
    // (LIVE == 1) keeps.
    if (a.q_delta != nullptr && valid) {
      T xq[N];
#pragma unroll
      for (int r = 0; r < N; ++r) xq[r] = XR_(r);
      // Written THROUGH the caches like the poses below: a consumer on another stream or a copy engine that reads them once
      // `done` has reached the tick must see this tick's results, not what an XCD's L2 still holds.  The pose rows are
      // [target][7]: a lane's own row is 56 bytes at a stride of 56, and written through as such every store is a partial line
      // straight to memory (configs[4]'s share: 4.9 -> 10.5 us per tick).  The wavefront's 64 rows are one contiguous run of
      // 3584 bytes, so they go through its LDS and leave as seven full 512-byte stores.
      double qd, qp[7];
      sphere_query_values<M, T>(xq, true, 0.0, a.q_origin, a.q_radius, qd, qp, a.q_pose != nullptr);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(&a.q_delta[entry]), (unsigned long long)__double_as_longlong(qd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (a.q_pose != nullptr) {
#pragma unroll
        for (int k = 0; k < 7; ++k) qpose_lds[lane * 7 + k] = qp[k];
      }
    }
    if (a.q_delta != nullptr && a.q_pose != nullptr) {   // (uniform) every lane takes part in the transposed store
      wave_lds_fence();
      const long first = wg * TPW;                                        // first target of this wavefront
      const long words = (a.n - first < TPW ? a.n - first : (long)TPW) * 7;   // its rows, as one run of words
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int f = k * 64 + lane;
        if (f < words)
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(&a.q_pose[first * 7 + f]), (unsigned long long)__double_as_longlong(qpose_lds[f]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      wave_lds_fence();
    }
    if (a.live_pose != nullptr) {   // the tick's estimated poses for a consumer outside the kernel (StepArgs::live_pose)
      if (valid) {
        T xq[N], pose7[7], twist6[6], acc6[6];
#pragma unroll
        for (int r = 0; r < N; ++r) xq[r] = XR_(r);
        derive_outputs<M, T>(xq, false, (T)0, pose7, twist6, acc6);
#pragma unroll
        for (int c = 0; c < 7; ++c)   // system-scope stores: written through to memory, 512 contiguous bytes per wavefront and row
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(&a.live_pose[(long)c * a.live_pose_ld + entry]),
                             (unsigned long long)__double_as_longlong((double)pose7[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tick's outputs have left before the progress word says so
  }
  if constexpr (POSE && FUSED) write_pose(tick);
  if constexpr (LIVE) {
    // tick `tick` is done (state in registers): a word in device memory for the relay
    if (lane == 0) {
      if (a.live_flags & kLiveWorkerRel) __hip_atomic_store(&a.live_progress[wave_id], tick + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_store(&a.live_progress[wave_id], tick + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (see kf_step.hpp, "Ordering of the hand-offs")
    }
  }
  }  // tick loop
  // FGATE: what follows the loop reads its arguments afresh as well (behind the loop: nothing of it is held across)
  SegByte* ke0 = FGATE ? (SegByte*)__builtin_amdgcn_kernarg_segment_ptr() : nullptr;
  if constexpr (FGATE) asm volatile("" : "+s"(ke0));
  FusedSeg* ke = (FusedSeg*)(ke0 + (FGATE ? SEG : 0u));
  (void)ke;
  if constexpr (UT) {
    // Does the tile leave this tick uniform?  Its lanes must have taken the same has-bit (dt is the launch's).  A uniform tile
    // then stays one -- every lane has computed the same block from the same block -- and a tile that is not becomes one, in a
    // launch that asks for it, if its valid lanes are found to agree on every linear P word, bit for bit.
    if (a.tile_uni != nullptr) {
      bool agree = true;
      if (a.has_meas != nullptr || (GATE && gate != 0.0)) agree = __all(!valid || n_has == __builtin_amdgcn_readfirstlane(n_has)) != 0;
      if (uni) {
        uni_out = agree;
      } else if (a.promote != 0 && agree) {
        bool same = true;
#pragma unroll
        for (int k = 0; k < C::LW; ++k) {
          const long long b = __double_as_longlong(mem[C::LIN.w[k]]);
          same = same && b == wave_uniform_ll(b);
        }
        uni_out = __all(!valid || same) != 0;
      }
    }
  }
  if (valid) {
    if constexpr (NPARK > 0) {   // the reverse of the session's first lines: chunk by chunk from the record's two homes
      using V = typename Vec16<T>::type;
#pragma unroll
      for (int c = 0; c < C::NC; ++c) {
        T w2[C::VW];
#pragma unroll
        for (int k = 0; k < C::VW; ++k) {
          const int w = c * C::VW + k;
          w2[k] = Park::SLOT.v[w] >= 0 ? park_lds[Park::SLOT.v[w] * 64 + lane] : mem[w];
        }
        V v;
        __builtin_memcpy(&v, w2, 16);
        *reinterpret_cast<V*>(tb + (long)c * C::LPT * 16 + (long)lt * 16) = v;
        if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (C::REM1)
        *reinterpret_cast<T*>(tb + C::TAIL1_OFF + (long)lt * (long)sizeof(T)) =
            Park::SLOT.v[C::RW - 1] >= 0 ? park_lds[Park::SLOT.v[C::RW - 1] * 64 + lane] : mem[C::RW - 1];
    }
    else if constexpr (UT) {
      char* dst = AB ? a.rec_out + tile * C::TILE_BYTES : tb;
      if (uni_out) {   // (wave-uniform) the tile's one block instead of 64 copies of it
        store_record_nonlin<C, T, AB>(dst, lt, mem);
        if (lane == 0) {   // (lane 0 of a dense wavefront that got here is valid)
#pragma unroll
          for (int k = 0; k < C::LW; ++k) a.tile_blk[tile * C::LW + k] = mem[C::LIN.w[k]];
          if (!uni) a.tile_uni[tile] = 1;
        }
      } else {
        if constexpr (AB) store_record<C, T, false, true>(dst, lt, mem);
        else store_record<C, T>(dst, lt, mem);
        if (uni && lane == 0) a.tile_uni[tile] = 0;
      }
    }
    else if constexpr (AB) store_record<C, T, false, true>(a.rec_out + tile * C::TILE_BYTES, lt, mem);   // A -> B tick (StepArgs::rec_out)
    else store_record<C, T>(tb, lt, mem);
    if constexpr (POSE && !FUSED) write_pose(0);
    if constexpr (LGATE) {   // the session's runs go back with its records
      if (lg->k >= 0) lg->run[entry] = (unsigned char)live_run;
    }
    else if constexpr (FGATE) {   // ... and the fused call's (its rows were written tick by tick)
      if (ke->g.k >= 0) ke->g.run[entry] = (unsigned char)live_run;
    }
    else if constexpr (GATE) write_innov(g_has, nis, nu_all, MI);
    else if constexpr (INNOV) write_innov(n_has != 0, nis, nu_all, MI);
    if constexpr (BYID && !TAIL_REGS) {
      if (by_reinit) {   // the record once more, behind store_record, as init_kernel / reacquire_kernel write it
        T x0[N];
#pragma unroll
        for (int r = 0; r < N; ++r) x0[r] = 0;
        if constexpr (M::ANGULAR) {
          T p6[6];
          pose7_to_pose6(by_y, p6);
#pragma unroll
          for (int c6 = 0; c6 < 6; ++c6) x0[c6] = p6[c6];
        } else {
#pragma unroll
          for (int c3 = 0; c3 < 3; ++c3) x0[c3] = by_y[c3];
        }
#pragma unroll
        for (int r = 0; r < N; ++r) {
          state_set<C, T>(a.rec, slot_of, r, N, x0[r]);
          XW_(r) = x0[r];   // (the getter-table row below reads the state words in registers)
        }
        const double* P0 = gid->p0_tab + (long)gid->p0_idx[slot_of] * N * N;
        for (int r = 0; r < N; ++r)
          for (int c = (C::SEPPK ? r : 0); c < N; ++c) state_set<C, T>(a.rec, slot_of, r, c, (T)P0[r * N + c]);
        if constexpr (M::ANGULAR) {
          for (int cc = 0; cc < 3; ++cc) *unwrap_ptr<C, T>(a.rec, slot_of, cc) = 0;
        }
      }
    }
    if constexpr (QUERY) {
      T xq[N];
#pragma unroll
      for (int r = 0; r < N; ++r) xq[r] = XW_(r);
      double qd, qp[7];
#ifdef TE_QUERY_PHASE_CLOCK
      long long ts[8];
      __builtin_amdgcn_sched_barrier(0); ts[0] = (long long)__builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0);
      sphere_query_values<M, T>(xq, true, 0.0, a.q_origin, a.q_radius, qd, qp, a.q_pose != nullptr, ts);
      // lanes 0..4 of every wavefront report: cycles from the wavefront's first instruction to the head of the query, then the query's phases
      qd = lane == 0 ? (double)(ts[0] - ts_begin) : lane == 1 ? (double)(ts[1] - ts[0]) : lane == 2 ? (double)(ts[2] - ts[1]) : lane == 3 ? (double)(ts[3] - ts[2]) : qd;
#else
      sphere_query_values<M, T>(xq, true, 0.0, a.q_origin, a.q_radius, qd, qp, a.q_pose != nullptr);
#endif
      a.q_delta[entry] = qd;
      if (a.q_pose != nullptr) {
#pragma unroll
        for (int k = 0; k < 7; ++k) a.q_pose[entry * 7 + k] = qp[k];
      }
    }
    if constexpr (INDEXED) {
      const long slot = slot_of;
      a.t_base[slot] = te_clock_add_ticks(a.t_base[slot], dtd, (double)n_ticks);
      a.nm_base[slot] += n_has;
    } else {
      if constexpr (FGATE) {   // (the gate read where it arrived: not a scalar register pair held across the tick loop)
        if (ke->a.has_meas != nullptr || ke->g.gate != 0.0) ke->a.nm_base[entry] += n_has;
      } else if (a.has_meas != nullptr || (GATE && gate != 0.0)) a.nm_base[entry] += n_has;
    }
  }
  if constexpr (INDEXED) {
    if (a.o_pose != nullptr) {   // uniform: the getter table and the completion flag in the same launch (StepArgs::o_pose)
      if (valid) {
        T xq[N];
#pragma unroll
        for (int r = 0; r < N; ++r) xq[r] = XW_(r);
        write_outputs_row<M, T>(xq, slot_of, a.o_pose, a.o_twist, a.o_acc);
      }
      signal_done(a.done_flag, a.done_seq, lane, a.done_count, a.n, TPW);
    }
  }
#undef XW_
#undef TE_EKF_JACOBIAN_
#undef GR_
#undef GATE_T_
#undef PG_
#undef A_
#undef FG0_
#undef FSEG_
#undef GW_
#undef UWW_
#undef XR_
#undef XS_
}

template <class M, typename T, int LAYOUT, unsigned VAR>
__global__ void __launch_bounds__(256, (sep_min_waves<M, T, LAYOUT, sv_has(VAR, kPerQR), sv_live(VAR)>())) kf_step_sep_kernel(const StepArgs<T> a) {
  unsigned b = blockIdx.x;
  if constexpr (!sv_has(VAR, kIndexed | kFused | kLiveMask)) {
    // zig-zag traversal (StepArgs::reverse): the workgroups, class by class (zigzag_map.hpp).  A select, not a branch: behind a
    // branch the load of the grid size waits for the one of `reverse` (10^5 UA fp32, never reversed: 5.7 -> 5.9 us per tick)
    const unsigned zz = zz_block(b, gridDim.x);
    b = a.reverse ? zz : b;
  }
  sep_step_wave<M, T, LAYOUT, VAR>(a, (long)b * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63));
}

// The gated tick (sep_step_wave, GATE): the kInnov kernel with the two-phase body and the gate as an argument of its own.
// Instantiated in kf_gate_{uv,ua,ar,av}.hip (kf_gate_impl.hpp).
template <class M, typename T, int LAYOUT>
__global__ void __launch_bounds__(256) kf_step_sep_gate_kernel(const StepArgs<T> a, const double gate) {
  unsigned b = blockIdx.x;
  const unsigned zz = zz_block(b, gridDim.x);
  b = a.reverse ? zz : b;
  sep_step_wave<M, T, LAYOUT, kInnov, true>(a, (long)b * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63), gate);
}

// The gated by-id tick (sep_step_wave, GATE + BYID): the kInnov | kIndexed step with the policy tail, everything new in the second
// argument -- StepArgs keeps its size.  Instantiated in kf_gate_id_{uv,ua,ar,av}.hip (kf_gate_id_impl.hpp).
template <class M, typename T, int LAYOUT>
__global__ void __launch_bounds__(256) kf_step_sep_gate_indexed_kernel(const StepArgs<T> a, const GateById g) {
  sep_step_wave<M, T, LAYOUT, kInnov | kIndexed, true, true>(a, (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63), g.gate, &g);
}

// The gated resident session (sep_step_wave, GATE inside the kFused | kLive2 tick loop; LiveGate above): the third resident
// instantiation.  Everything new travels in the second argument -- StepArgs keeps its size -- and the plain and pose / query
// sessions keep their kernels.  Never held to a register limit (see sep_min_waves: a resident kernel must not spill); what the
// gate's values between the two phases cost in wavefronts per SIMD is in profiles/live_gate_kernel_resources.txt, and
// OpsImpl::live_capacity asks the occupancy query about THIS kernel.  Instantiated in kf_live_gate_{uv,ua,ar,av}.hip
// (kf_live_gate_impl.hpp), packed groups only (the layout that has resident kernels).
template <class M, typename T, int LAYOUT>
__global__ void __launch_bounds__(256) kf_step_sep_live_gate_kernel(const StepArgs<T> a, const LiveGate g) {
  // `g` where the launch put it: explicit kernel arguments lie in the segment in order, each at its natural alignment
  constexpr unsigned long G_OFF = (sizeof(StepArgs<T>) + alignof(LiveGate) - 1) / alignof(LiveGate) * alignof(LiveGate);
  typedef const char __attribute__((address_space(4))) ArgByte;
  LiveGateArg* gp = (LiveGateArg*)((ArgByte*)__builtin_amdgcn_kernarg_segment_ptr() + G_OFF);
  sep_step_wave<M, T, LAYOUT, kFused | kLive2, true, false>(a, (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63), g.gate, nullptr, gp);
}

// The launched fused call with the gate inside (sep_step_wave, GATE inside the plain kFused tick loop; FusedGate above):
// target_batch_step_fused_gated.  Everything new travels in the second argument -- StepArgs keeps its size -- and the plain kFused
// kernels stay what they were.  Nothing here waits: no atomic read-modify-write, no word shared between wavefronts.  Instantiated in
// kf_fused_gate_{uv,ua,ar,av}.hip (kf_fused_gate_impl.hpp) for the two separable layouts in both precisions; the grid is the
// plain fused launch's.
template <class M, typename T, int LAYOUT>
__global__ void __launch_bounds__(256) kf_step_sep_fused_gate_kernel(const StepArgs<T> a, const FusedGate g) {
  // sep_step_wave reads `g` where the launch put it (FusedGateSegment; see kf_step_sep_live_gate_kernel)
  static_assert(offsetof(FusedGateSegment<T>, g) == (sizeof(StepArgs<T>) + alignof(FusedGate) - 1) / alignof(FusedGate) * alignof(FusedGate),
                "explicit kernel arguments lie in the segment in order, each at its natural alignment");
  sep_step_wave<M, T, LAYOUT, kFused, true, false>(a, (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63), g.gate);
}

// The launched fused calls with a time-step schedule (sep_step_wave, DTTAB): target_batch_step_fused_dt.  dt_tab [a.n_ticks] doubles in
// device memory, written on the stream ahead of the launch and never while it runs; StepArgs::dt is not read.  The plain loop and
// the gated one, each the kernel above it with the table as one more argument -- StepArgs and FusedGate keep their sizes.  Instantiated
// in kf_fused_dt_{uv,ua,ar,av}.hip (kf_fused_dt_impl.hpp) for the two separable layouts in both precisions; the grids are the plain
// fused launch's.
template <class M, typename T, int LAYOUT>
__global__ void __launch_bounds__(256, (sep_min_waves<M, T, LAYOUT, false, 0>())) kf_step_sep_fused_dt_kernel(const StepArgs<T> a, const double* dt_tab) {
  sep_step_wave<M, T, LAYOUT, kFused, false, false, true>(a, (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63), 0.0, nullptr,
                                                          nullptr, dt_tab);
}
template <class M, typename T, int LAYOUT>
__global__ void __launch_bounds__(256) kf_step_sep_fused_gate_dt_kernel(const StepArgs<T> a, const FusedGate g, const double* dt_tab) {
  static_assert(offsetof(FusedGateDtSegment<T>, g) == offsetof(FusedGateSegment<T>, g) &&
                    offsetof(FusedGateDtSegment<T>, dt_tab) == (offsetof(FusedGateSegment<T>, g) + sizeof(FusedGate) + 7) / 8 * 8,
                "explicit kernel arguments lie in the segment in order, each at its natural alignment");
  (void)dt_tab;   // (sep_step_wave reads it where the launch put it, tick by tick)
  sep_step_wave<M, T, LAYOUT, kFused, true, false, true>(a, (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63), g.gate);
}

// ---- one launch for the whole population of a manager ------------------------------------------------------------------------
// A manager with several motion models has one batch per model; their ticks are independent, and as separate launches they only
// overlap if the runtime happens to put their streams on hardware queues that the device runs side by side.  That is not a
// property to build on: measured (profiles/r04_queue_pipes.txt), the two branches of a recorded tick ran 2-3x slower as soon as
// the process owned a fifth hardware queue, whoever created it.  Here the tick of ALL batches is one grid: the first end[0]
// workgroups step the angular-rates batch, the next ones the angular-velocities batch, and so on in the order of the
// reference's enum (target_manager.hpp:38) -- the heaviest model first (measured at configs[4]'s share: light parts first 13.6 -> 15.2 us
// per tick, the two parts' workgroups alternating 14.9; gpurun_out/r4popgrid).  Each part is exactly kf_step_sep_kernel's arithmetic
// (sep_step_wave) on its own StepArgs; an absent model has end[k] == end[k - 1].
// POSE: every part with a non-null StepArgs::pose also writes the tick's poses (sep_step_wave, POSE); a part without one (null)
// skips that on a wavefront-uniform branch.  The POSE instantiations live in kf_population_f{64,32}_pose.hip.
template <typename T>
struct PopulationArgs {
  StepArgs<T> part[4];     // indexed by ModelType
  unsigned end[4];         // first workgroup BEHIND part k
  int reverse_blocks;      // zig-zag over the whole population: walk the workgroups (parts and their tiles) last to first, class by class (zigzag_map.hpp)
};

// SHARED: every part is a batch in the shared-axes storage form (te_layout.hpp LAYOUT_SEPARABLE_SHARED; fp64 only).
// INNOV: every part with a non-null StepArgs::nis also writes the tick's innovation stream (sep_step_wave, INNOV); in place, without
// the fused query or the pose output.  Instantiated in kf_population_f{64,32}_innov.hip and kf_population_f64_shared_innov.hip.
// VAR: kQuery, kAB, kPose, kInnov of the variant word, handed to every part's sep_step_wave.
template <typename T, bool SHARED, unsigned VAR>
__global__ void __launch_bounds__(256) kf_step_population_kernel(const PopulationArgs<T> p) {
  static_assert(population_variant_ok(VAR, SHARED), "no such variant of the population step (step_variant.hpp)");
  const int lane = (int)(threadIdx.x & 63);
  const unsigned wpb = blockDim.x >> 6, wave = threadIdx.x >> 6;
  unsigned b = blockIdx.x;
  if (p.reverse_blocks) b = zz_block(b, gridDim.x);
  constexpr int L = SHARED ? LAYOUT_SEPARABLE_SHARED : LAYOUT_SEPARABLE_PACKED;
  if (b < p.end[0]) sep_step_wave<ModelAR, T, L, VAR>(p.part[0], (long)b * wpb + wave, lane);
  else if (b < p.end[1]) sep_step_wave<ModelAV, T, L, VAR>(p.part[1], (long)(b - p.end[0]) * wpb + wave, lane);
  else if (b < p.end[2]) sep_step_wave<ModelUA, T, L, VAR>(p.part[2], (long)(b - p.end[1]) * wpb + wave, lane);
  else sep_step_wave<ModelUV, T, L, VAR>(p.part[3], (long)(b - p.end[2]) * wpb + wave, lane);
}

// The population tick with the gated body (sep_step_wave, GATE): gate[k] is part k's nis_max, 0 = that part has no gate and
// leaves in the bits of the kInnov tick.  Instantiated in kf_population_f{64,32}_gate.hip and kf_population_f64_shared_gate.hip.
struct PopulationGate {
  double gate[4];   // indexed by ModelType, like PopulationArgs::part
};
template <typename T, bool SHARED>
__global__ void __launch_bounds__(256) kf_step_population_gate_kernel(const PopulationArgs<T> p, const PopulationGate g) {
  const int lane = (int)(threadIdx.x & 63);
  const unsigned wpb = blockDim.x >> 6, wave = threadIdx.x >> 6;
  unsigned b = blockIdx.x;
  if (p.reverse_blocks) b = zz_block(b, gridDim.x);
  constexpr int L = SHARED ? LAYOUT_SEPARABLE_SHARED : LAYOUT_SEPARABLE_PACKED;
  if (b < p.end[0]) sep_step_wave<ModelAR, T, L, kInnov, true>(p.part[0], (long)b * wpb + wave, lane, g.gate[0]);
  else if (b < p.end[1]) sep_step_wave<ModelAV, T, L, kInnov, true>(p.part[1], (long)(b - p.end[0]) * wpb + wave, lane, g.gate[1]);
  else if (b < p.end[2]) sep_step_wave<ModelUA, T, L, kInnov, true>(p.part[2], (long)(b - p.end[1]) * wpb + wave, lane, g.gate[2]);
  else sep_step_wave<ModelUV, T, L, kInnov, true>(p.part[3], (long)(b - p.end[2]) * wpb + wave, lane, g.gate[3]);
}

// ---- one launch for a temporally fused replay of the whole population ------------------------------------------------------------
// The launched fused loops (sep_step_wave, kFused; with GATE the loop of kf_step_sep_fused_gate_kernel, with DTTAB the schedule's
// table) on the population grid: the first end[0] workgroups run the angular-rates batch's whole call, the next ones the
// angular-velocities batch's, and so on -- the split of kf_step_population_kernel, never reversed (a fused call walks its tiles
// once).  Each part is exactly its per-batch kernel's arithmetic on its own arguments; the plain form of the separable layout with
// packed groups only (the host expands a shared-axes batch first, as for every fused call).
// The ONE kernel argument is, for every instantiation, four FusedGateDtSegment -- what the per-batch gated kernel with a table finds
// at offset 0 of its segment -- followed by the grid split: the gated loop of part k reads its arguments per tick at the
// compile-time offset k * sizeof(FusedGateDtSegment<T>) (sep_step_wave, SEG), the plain loops take part[k].a by reference and (DTTAB)
// part[k].dt_tab by value.  Every part carries the call's one table.  A part without a gate has gate 0 (acc = has), one without a
// policy k = -1; in a gated launch every non-empty part has NIS rows (the host's rule: Shard::stepFusedAll).
// (the struct itself and the offset of part k are stated in step_variant.hpp, where a host test holds them to offsetof)
template <typename T>
using PopulationFusedArgs = PopulationFusedLayout<FusedGateDtSegment<T>>;
static_assert(population_fused_args_fit<FusedGateDtSegment<double>>() && population_fused_args_fit<FusedGateDtSegment<float>>(),
              "the arguments of a kernel are at most 4 KB");
template <typename T>
constexpr unsigned population_fused_seg(int k) { return population_fused_seg_offset<FusedGateDtSegment<T>>(k); }
static_assert(offsetof(PopulationFusedArgs<double>, part[3].g) == population_fused_seg<double>(3) + offsetof(FusedGateSegment<double>, g) &&
                  offsetof(PopulationFusedArgs<float>, part[1].dt_tab) == population_fused_seg<float>(1) + offsetof(FusedGateDtSegment<float>, dt_tab),
              "part k of the argument struct lies where sep_step_wave's SEG says");

template <typename T, bool GATE, bool DTTAB>
__global__ void __launch_bounds__(256) kf_step_population_fused_kernel(const PopulationFusedArgs<T> p) {
  const int lane = (int)(threadIdx.x & 63);
  const unsigned wpb = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const unsigned b = blockIdx.x;
  constexpr int L = LAYOUT_SEPARABLE_PACKED;
#define TE_POP_FUSED_PART_(k_, Model_, first_)                                                                                       \
  sep_step_wave<Model_, T, L, kFused, GATE, false, DTTAB, population_fused_seg<T>(k_)>(p.part[k_].a, (long)(b - (first_)) * wpb + wave, lane, \
                                                                                      p.part[k_].g.gate, nullptr, nullptr, p.part[k_].dt_tab)
  if (b < p.end[0]) TE_POP_FUSED_PART_(0, ModelAR, 0u);
  else if (b < p.end[1]) TE_POP_FUSED_PART_(1, ModelAV, p.end[0]);
  else if (b < p.end[2]) TE_POP_FUSED_PART_(2, ModelUA, p.end[1]);
  else TE_POP_FUSED_PART_(3, ModelUV, p.end[2]);
#undef TE_POP_FUSED_PART_
}

}  // namespace te
