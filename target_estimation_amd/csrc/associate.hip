// associate.hip -- the association kernels: a table row per target, the two pair scans, the resolve step, the scatter (associate.hpp;
// DESIGN.md 3.18).  A unit of its own: no step kernel is touched.
#include "associate.hpp"

#include "crossing_cov_plan.hpp"
#include "hip_check.hpp"
#include "kf_aux.hpp"

namespace te {

// A thread per slot.  zhat = the position derive_outputs gives at the offset dt; Sigma = (A(dt) P A(dt)^T + Q)[0:3, 0:3] exactly as
// crossing_cov_kernel forms it (crossing_predict_block per stored pair, the layout's accessors, a flagged uniform tile's words from
// the tile's block, exact zeros between the axes of the separable layouts), in the batch's precision; S = Sigma + R[0:3, 0:3] of the
// slot's class and W = S^-1 in double (assoc_invert_s).  An invalid S gives a NaN row: never a candidate.  With a.sigma_in_w the
// row's six W words receive Sigma itself, the doubles above before R is added (a MergeRow: track_merge_plan.hpp); validity as before.
template <class M, typename T, int G, int LAYOUT>
__global__ __launch_bounds__(64) void assoc_table_kernel(const AssocTableArgs a) {
#pragma clang fp contract(off)
  using C = Cfg<M, T, G, LAYOUT>;
  constexpr int N = C::N, K = C::K, NB = C::NB;
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= a.size) return;
  const T tau = (T)a.dt;
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
  double S[6], Sg[6];   // Sg: Sigma before R is added (the track-merge row)
#pragma unroll
  for (int r = 0, k = 0; r < 3; ++r) {
#pragma unroll
    for (int c = r; c < 3; ++c, ++k) {
      const int rw = C::RWORD.v[r][c];
      const double Rrc = rw >= 0 ? (double)qr[rw] : 0.0;
      if (C::SEP && r != c) { Sg[k] = 0.0; S[k] = 0.0 + Rrc; continue; }
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
      Sg[k] = (double)B[0][0];
      S[k] = (double)B[0][0] + Rrc;
    }
  }
  T x[N];
#pragma unroll
  for (int r = 0; r < N; ++r) x[r] = state_get<C, T>(a.rec, slot, r, N);
  T pose7[7], twist6[6], acc6[6];
  derive_outputs<M, T>(x, true, tau, pose7, twist6, acc6);
  double W[6];
  const bool ok = assoc_invert_s(S, W);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double* row = reinterpret_cast<double*>(a.rows + slot);
#pragma unroll
  for (int c = 0; c < 3; ++c) row[c] = ok ? (double)pose7[c] : nan;
#pragma unroll
  for (int k = 0; k < 6; ++k) row[3 + k] = a.sigma_in_w ? Sg[k] : W[k];
  reinterpret_cast<long long*>(row)[9] = ((long long)a.batch_index << 32) | (long long)(unsigned)slot;
  if (a.sdiag) {   // the grid form (associate_grid.hpp): the diagonal of the S that was just inverted
    a.sdiag[slot * 3] = S[0]; a.sdiag[slot * 3 + 1] = S[3]; a.sdiag[slot * 3 + 2] = S[5];
  }
}

struct AssocScanArgs {
  const AssocRow* table;
  const double* det;      // [M][7]
  const int* det_of_row;
  const int* row_of_det;
  const int* state;
  long rows, M;
  double gate;
  AssocGrid grid;         // of THIS scan: rows = what the threads own, cols = what they walk
  double* part_d2;        // [chunks][grid.rows]
  int* part_idx;
};

__global__ void assoc_init_kernel(long rows, long M, int* det_of_row, double* d2_of_row, int* row_of_det, double* d2_of_det, int* state) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) { det_of_row[i] = -1; d2_of_row[i] = -1.0; }
  if (i < M) { row_of_det[i] = -1; d2_of_det[i] = -1.0; }
  if (i == 0) { state[0] = 0; state[1] = 0; state[2] = (rows == 0 || M == 0) ? 1 : 0; state[3] = 0; }
}

// TARGET-MAJOR.  Workgroup (x, y) owns rows x * kAssocTile .. and walks the detections of chunk y in ascending order, a tile of
// kAssocTile detections at a time through LDS (a matched detection is staged as NaN: the candidate rule rejects it).  Every lane
// reads the same LDS word: a broadcast.  A matched row, a NaN row and a row beyond the table walk nothing.
__global__ __launch_bounds__(kAssocTile) void assoc_scan_rows_kernel(const AssocScanArgs a) {
#pragma clang fp contract(off)
  if (a.state[2] != 0) return;   // (the whole grid reads the same word: settled by an earlier round)
  __shared__ double s_det[3][kAssocTile];
  const int tid = (int)threadIdx.x, chunk = (int)blockIdx.y;
  const long row = (long)blockIdx.x * kAssocTile + tid;
  const long c0 = a.grid.col_begin(chunk), c1 = a.grid.col_end(chunk);
  bool active = row < a.rows && a.det_of_row[row] < 0;
  double zh[3] = {0.0, 0.0, 0.0}, W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (active) {
    const double* r = reinterpret_cast<const double*>(a.table + row);
#pragma unroll
    for (int c = 0; c < 3; ++c) zh[c] = r[c];
#pragma unroll
    for (int k = 0; k < 6; ++k) W[k] = r[3 + k];
    active = zh[0] == zh[0];
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  AssocBest best = assoc_best_none();
  for (long base = c0; base < c1; base += kAssocTile) {
    const long j = base + tid;
    double x = nan, y = nan, z = nan;
    if (j < c1 && a.row_of_det[j] < 0) { x = a.det[j * 7]; y = a.det[j * 7 + 1]; z = a.det[j * 7 + 2]; }
    __syncthreads();   // the tile before this one has been read
    s_det[0][tid] = x; s_det[1][tid] = y; s_det[2][tid] = z;
    __syncthreads();
    const int cnt = (int)((c1 - base) < (long)kAssocTile ? (c1 - base) : (long)kAssocTile);
    if (active) {
#pragma unroll 4
      for (int t = 0; t < cnt; ++t) {
        const double d2 = assoc_d2(zh, W, s_det[0][t], s_det[1][t], s_det[2][t]);
        if (assoc_candidate(d2, a.gate)) assoc_take(best, d2, (int)(base + t));
      }
    }
  }
  if (row < a.rows) {
    a.part_d2[(long)chunk * a.rows + row] = best.d2;
    a.part_idx[(long)chunk * a.rows + row] = best.idx;
  }
}

// DETECTION-MAJOR, the mirror image.  Workgroup (x, y) owns detections x * kAssocTile .. and walks the table rows of chunk y in
// ascending order -- (batch, slot) order -- a tile of kAssocTile rows at a time through LDS, 80 B per row, copied as they lie (a
// coalesced copy); a matched row's zhat[0] is then overwritten with NaN in LDS.
__global__ __launch_bounds__(kAssocTile) void assoc_scan_dets_kernel(const AssocScanArgs a) {
#pragma clang fp contract(off)
  if (a.state[2] != 0) return;
  __shared__ double s_row[kAssocTile * kAssocRowWords];
  const int tid = (int)threadIdx.x, chunk = (int)blockIdx.y;
  const long j = (long)blockIdx.x * kAssocTile + tid;
  const long c0 = a.grid.col_begin(chunk), c1 = a.grid.col_end(chunk);
  bool active = j < a.M && a.row_of_det[j] < 0;
  double x = 0.0, y = 0.0, z = 0.0;
  if (active) {
    x = a.det[j * 7]; y = a.det[j * 7 + 1]; z = a.det[j * 7 + 2];
    active = x == x && y == y && z == z;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double* table = reinterpret_cast<const double*>(a.table);
  AssocBest best = assoc_best_none();
  for (long base = c0; base < c1; base += kAssocTile) {
    const int cnt = (int)((c1 - base) < (long)kAssocTile ? (c1 - base) : (long)kAssocTile);
    __syncthreads();   // the tile before this one has been read
#pragma unroll
    for (int k = 0; k < kAssocRowWords; ++k) {
      const int w = k * kAssocTile + tid;
      if (w < cnt * kAssocRowWords) s_row[w] = table[base * kAssocRowWords + w];
    }
    __syncthreads();
    if (tid < cnt && a.det_of_row[base + tid] >= 0) s_row[tid * kAssocRowWords] = nan;
    __syncthreads();
    if (active) {
#pragma unroll 2
      for (int t = 0; t < cnt; ++t) {
        const double* r = s_row + t * kAssocRowWords;
        const double d2 = assoc_d2(r, r + 3, x, y, z);
        if (assoc_candidate(d2, a.gate)) assoc_take(best, d2, (int)(base + t));
      }
    }
  }
  if (j < a.M) {
    a.part_d2[(long)chunk * a.M + j] = best.d2;
    a.part_idx[(long)chunk * a.M + j] = best.idx;
  }
}

struct AssocResolveArgs {
  long rows, M;
  int chunks_rows, chunks_dets;   // of the target-major and the detection-major scan
  const double* part_rows_d2;
  const int* part_rows_idx;
  const double* part_dets_d2;
  const int* part_dets_idx;
  int* det_of_row;
  double* d2_of_row;
  int* row_of_det;
  double* d2_of_det;
  int* state;
};

// ONE workgroup, a thread per unmatched detection (M <= 65536: at most 64 per thread).  The detection's pick is the merge of its
// partials; if that row's pick -- the merge of the row's partials -- is this detection, the two are matched: one writer per word,
// since a row is picked back by one detection only.  d2_of_row is the target-major scan's value, d2_of_det the detection-major
// scan's.  Then the counts: matched += ..., rounds_run += 1, settled = no detection that had a candidate stayed unmatched.
constexpr int kAssocResolveThreads = 1024;
__global__ __launch_bounds__(kAssocResolveThreads) void assoc_resolve_kernel(const AssocResolveArgs a) {
  if (a.state[2] != 0) return;
  __shared__ int s_matched[kAssocResolveThreads / 64], s_open[kAssocResolveThreads / 64];
  const int tid = (int)threadIdx.x;
  int matched = 0, open = 0;
  for (long j = tid; j < a.M; j += kAssocResolveThreads) {
    if (a.row_of_det[j] >= 0) continue;
    const AssocBest bd = assoc_merge(a.part_dets_d2, a.part_dets_idx, a.M, a.chunks_dets, j);
    if (bd.idx < 0) continue;
    const long i = bd.idx;
    const AssocBest br = assoc_merge(a.part_rows_d2, a.part_rows_idx, a.rows, a.chunks_rows, i);
    if (br.idx == (int)j) {
      a.row_of_det[j] = (int)i; a.d2_of_det[j] = bd.d2;
      a.det_of_row[i] = (int)j; a.d2_of_row[i] = br.d2;
      ++matched;
    } else {
      ++open;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { matched += __shfl_down(matched, o, 64); open += __shfl_down(open, o, 64); }
  if ((tid & 63) == 0) { s_matched[tid >> 6] = matched; s_open[tid >> 6] = open; }
  __syncthreads();
  if (tid == 0) {
    int m = 0, o = 0;
    for (int w = 0; w < kAssocResolveThreads / 64; ++w) { m += s_matched[w]; o += s_open[w]; }
    a.state[0] += m;
    a.state[1] += 1;
    a.state[2] = o == 0 ? 1 : 0;
  }
}

// A thread per slot of one batch: a matched slot gets its detection's 7 words rounded once to the batch's precision, an unmatched
// one the identity pose [0 0 0 0 0 0 1]; the mask; the detection index and the target-major d^2.
template <typename T>
__global__ void assoc_scatter_kernel(long row_offset, long size, const double* det, const int* det_of_row, const double* d2_of_row,
                                     T* meas, long ld, unsigned char* has_meas, int* det_of_slot, double* d2_of_slot) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= size) return;
  const int j = det_of_row[row_offset + slot];
  if (meas) {
#pragma unroll
    for (int c = 0; c < 7; ++c) meas[(long)c * ld + slot] = j >= 0 ? (T)det[(long)j * 7 + c] : (T)(c == 6 ? 1 : 0);
  }
  if (has_meas) has_meas[slot] = j >= 0 ? 1 : 0;
  if (det_of_slot) det_of_slot[slot] = j;
  if (d2_of_slot) d2_of_slot[slot] = j >= 0 ? d2_of_row[row_offset + slot] : -1.0;
}

__global__ void assoc_dets_kernel(long M, const AssocRow* table, const int* row_of_det, const double* d2_src, const int* state,
                                  int* slot_of_det, int* batch_of_det, double* d2_of_det, int* info) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0 && info) { info[0] = state[0]; info[1] = state[1]; info[2] = state[2]; info[3] = 0; }
  if (j >= M) return;
  const int row = row_of_det[j];
  int slot = -1, batch = -1;
  if (row >= 0) {
    const long long tag = reinterpret_cast<const long long*>(table + row)[9];
    slot = (int)(unsigned)(tag & 0xffffffffll);
    batch = (int)(tag >> 32);
  }
  if (slot_of_det) slot_of_det[j] = slot;
  if (batch_of_det) batch_of_det[j] = batch;
  if (d2_of_det) d2_of_det[j] = row >= 0 ? d2_src[j] : -1.0;
}

// ---------------------------------------------------------------- the scratch
// (a scratch carries nothing over: every block is released before its replacement exists, with its capacity at 0 meanwhile, so a
// throw leaves a scratch that the next call grows again.  A first call allocates every block, a call with a zero count included --
// the presence test is on the block of each group that is allocated last --, so no launch or copy is ever handed a null array)
void AssocScratch::ensure(long rows, long dets, long part_rows, long part_dets) {
  if (!state) state.alloc(4);
  if (rows > cap_rows_ || !d2_of_row) {
    const size_t want = rows > 64 ? rows : 64;
    cap_rows_ = 0;
    table.alloc(want); det_of_row.alloc(want); d2_of_row.alloc(want);
    cap_rows_ = (long)want;
  }
  if (dets > cap_dets_ || !d2_of_det) {
    const size_t want = dets > 64 ? dets : 64;
    cap_dets_ = 0;
    row_of_det.alloc(want); d2_of_det.alloc(want);
    cap_dets_ = (long)want;
  }
  if (part_rows > cap_part_rows_ || !part_rows_idx) {
    const size_t want = part_rows > 64 ? part_rows : 64;
    cap_part_rows_ = 0;
    part_rows_d2.alloc(want); part_rows_idx.alloc(want);
    cap_part_rows_ = (long)want;
  }
  if (part_dets > cap_part_dets_ || !part_dets_idx) {
    const size_t want = part_dets > 64 ? part_dets : 64;
    cap_part_dets_ = 0;
    part_dets_d2.alloc(want); part_dets_idx.alloc(want);
    cap_part_dets_ = (long)want;
  }
}

void AssocScratch::ensure_host(long dets) {
  if (dets <= cap_host_ && result_host) return;
  const size_t want = dets > 64 ? dets : 64;
  cap_host_ = 0;
  det_stage.alloc(want * 7);
  result_dev.alloc(result_bytes((long)want));
  result_host.alloc(result_bytes((long)want));
  cap_host_ = (long)want;
}

// ---------------------------------------------------------------- the launches
void launch_assoc_match(const AssocScratch& s, long rows, const double* det, long M, double gate, int rounds, int forced_chunks, hipStream_t st) {
  const long most = rows > M ? rows : M;
  hipLaunchKernelGGL(assoc_init_kernel, dim3((unsigned)((most + 255) / 256 > 0 ? (most + 255) / 256 : 1)), dim3(256), 0, st, rows, M,
                     s.det_of_row.get(), s.d2_of_row.get(), s.row_of_det.get(), s.d2_of_det.get(), s.state.get());
  if (rows <= 0 || M <= 0) return;   // (the state says settled, no round run)
  const AssocGrid gr = plan_assoc_grid(rows, M, forced_chunks);   // target-major: rows own, detections walked
  const AssocGrid gd = plan_assoc_grid(M, rows, forced_chunks);   // detection-major
  AssocScanArgs ar{s.table.get(), det, s.det_of_row.get(), s.row_of_det.get(), s.state.get(), rows, M, gate, gr, s.part_rows_d2.get(), s.part_rows_idx.get()};
  AssocScanArgs ad{s.table.get(), det, s.det_of_row.get(), s.row_of_det.get(), s.state.get(), rows, M, gate, gd, s.part_dets_d2.get(), s.part_dets_idx.get()};
  AssocResolveArgs rs{rows, M, gr.chunks, gd.chunks, s.part_rows_d2.get(), s.part_rows_idx.get(), s.part_dets_d2.get(), s.part_dets_idx.get(),
                      s.det_of_row.get(), s.d2_of_row.get(), s.row_of_det.get(), s.d2_of_det.get(), s.state.get()};
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(assoc_scan_rows_kernel, dim3((unsigned)gr.row_tiles, (unsigned)gr.chunks), dim3(kAssocTile), 0, st, ar);
    hipLaunchKernelGGL(assoc_scan_dets_kernel, dim3((unsigned)gd.row_tiles, (unsigned)gd.chunks), dim3(kAssocTile), 0, st, ad);
    hipLaunchKernelGGL(assoc_resolve_kernel, dim3(1), dim3(kAssocResolveThreads), 0, st, rs);
  }
}

void launch_assoc_scatter(int dtype, const AssocScratch& s, long row_offset, long size, const double* det, const AssocSlotOut& out, hipStream_t st) {
  if (size <= 0) return;
  const dim3 grid((unsigned)((size + 255) / 256)), block(256);
  if (dtype == F64)
    hipLaunchKernelGGL((assoc_scatter_kernel<double>), grid, block, 0, st, row_offset, size, det, s.det_of_row.get(), s.d2_of_row.get(),
                       static_cast<double*>(out.meas), out.ld, out.has_meas, out.det_of_slot, out.d2_of_slot);
  else if (dtype == F32)
    hipLaunchKernelGGL((assoc_scatter_kernel<float>), grid, block, 0, st, row_offset, size, det, s.det_of_row.get(), s.d2_of_row.get(),
                       static_cast<float*>(out.meas), out.ld, out.has_meas, out.det_of_slot, out.d2_of_slot);
  else
    throw std::logic_error("target_estimation_amd: associate: no scatter kernel for this precision");
}

void launch_assoc_dets(const AssocScratch& s, long M, int* slot_of_det, int* batch_of_det, double* d2_of_det, int* info, hipStream_t st) {
  hipLaunchKernelGGL(assoc_dets_kernel, dim3((unsigned)((M + 255) / 256 > 0 ? (M + 255) / 256 : 1)), dim3(256), 0, st, M, s.table.get(),
                     s.row_of_det.get(), s.d2_of_det.get(), s.state.get(), slot_of_det, batch_of_det, d2_of_det, info);
}

namespace {

template <class M, typename T, int G, int LAYOUT>
void launch_table(const AssocTableArgs& a, hipStream_t st) {
  if (a.size <= 0) return;
  hipLaunchKernelGGL((assoc_table_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.size + 63) / 64)), dim3(64), 0, st, a);
}

// every lanes-per-target count a model's layouts come in (te_layout.hpp: G divides K): the table of crossing_cov_launcher
template <class M, typename T>
AssocTableLaunch pick(int g, int layout, bool shared_axes) {
  if (shared_axes) {
    if constexpr (sizeof(T) == 8) return &launch_table<M, T, 1, LAYOUT_SEPARABLE_SHARED>;
    return nullptr;
  }
  if (layout == LAYOUT_SEPARABLE) return g == 1 ? &launch_table<M, T, 1, LAYOUT_SEPARABLE> : nullptr;
  if (layout == LAYOUT_SEPARABLE_PACKED) return g == 1 ? &launch_table<M, T, 1, LAYOUT_SEPARABLE_PACKED> : nullptr;
  if (layout == LAYOUT_FULL) {
    if (g == 1) return &launch_table<M, T, 1, LAYOUT_FULL>;
    if (g == 3) return &launch_table<M, T, 3, LAYOUT_FULL>;
    if constexpr (M::K == 6) {
      if (g == 2) return &launch_table<M, T, 2, LAYOUT_FULL>;
      if (g == 6) return &launch_table<M, T, 6, LAYOUT_FULL>;
    }
    return nullptr;
  }
  if (layout == LAYOUT_PACKED) {
    if (g == 1) return &launch_table<M, T, 1, LAYOUT_PACKED>;
    if (g == 3) return &launch_table<M, T, 3, LAYOUT_PACKED>;
    if constexpr (M::K == 6) {
      if (g == 2) return &launch_table<M, T, 2, LAYOUT_PACKED>;
      if (g == 6) return &launch_table<M, T, 6, LAYOUT_PACKED>;
    }
    return nullptr;
  }
  return nullptr;
}

template <class M>
AssocTableLaunch pick_dtype(int dtype, int g, int layout, bool shared_axes) {
  if (dtype == F64) return pick<M, double>(g, layout, shared_axes);
  if (dtype == F32) return pick<M, float>(g, layout, shared_axes);
  return nullptr;
}

}  // namespace

AssocTableLaunch assoc_table_launcher(int type, int dtype, int g, int layout, bool shared_axes) {
  switch (type) {
    case UNIFORM_VELOCITY: return pick_dtype<ModelUV>(dtype, g, layout, shared_axes);
    case UNIFORM_ACCELERATION: return pick_dtype<ModelUA>(dtype, g, layout, shared_axes);
    case ANGULAR_RATES: return pick_dtype<ModelAR>(dtype, g, layout, shared_axes);
    case ANGULAR_VELOCITIES: return pick_dtype<ModelAV>(dtype, g, layout, shared_axes);
  }
  return nullptr;
}

}  // namespace te
