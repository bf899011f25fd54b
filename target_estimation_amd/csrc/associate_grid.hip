// associate_grid.hip -- the kernels of the grid form of the association (associate_grid.hpp lists the launches; the rule is
// associate_grid_plan.hpp).  A unit of its own: the brute-force kernels (associate.hip) are not touched, and the
// scatter and the per-detection outputs are theirs.
#include "associate_grid.hpp"

#include "hip_check.hpp"

namespace te {

constexpr int kGT = kAssocGridThreads;
constexpr int kScanPerThread = 8;
constexpr int kScanPerBlock = kGT * kScanPerThread;   // counts a scan workgroup owns
constexpr int kWideWords = 12;                         // a wide row staged in LDS: zhat (3) | W (6) | reach2 (3)
constexpr int kWalkLanes = 32;                         // lanes that share ONE row's (detection's) walk: a lane per cell of the 27, five idle
constexpr int kWalkPerWg = kGT / kWalkLanes;           // rows (detections) a scan workgroup owns

struct AssocGridArgs {
  const AssocRow* table;
  const double* det;       // [M][7]
  const double* sdiag;     // [rows][3]
  double* reach2;          // [rows][3]
  int* bucket_of;          // [M] the detections' buckets, then [rows] the rows' (-1: binned nowhere)
  int* count;              // [hd + hr]: the detection buckets, then the row buckets
  int* start;              // [hd + hr + 1]
  int* cursor;             // [hd + hr]
  int* sums;               // the scan's block sums
  int* order;              // [M + rows]: the detections grouped by bucket, then the narrow rows grouped by bucket
  int* wide;               // [rows]: the wide rows, in no particular order
  int* counters;           // {wide rows, matched this round, open this round, 0}
  int* det_of_row;
  double* d2_of_row;
  int* row_of_det;
  double* d2_of_det;
  double* pick_row_d2;     // [rows]: this round's pick of every unmatched valid row
  int* pick_row_idx;
  double* pick_det_d2;     // [M]
  int* pick_det_idx;
  int* state;              // {matched, rounds_run, settled, 0}
  long rows, M;
  long hd, hr;             // buckets of the detections and of the rows: powers of two
  double gate, cell, lim2;
};

__global__ __launch_bounds__(kGT) void assoc_grid_init_kernel(const AssocGridArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.rows) { a.det_of_row[i] = -1; a.d2_of_row[i] = -1.0; a.pick_row_idx[i] = -1; a.pick_row_d2[i] = -1.0; }
  if (i < a.M) { a.row_of_det[i] = -1; a.d2_of_det[i] = -1.0; a.pick_det_idx[i] = -1; a.pick_det_d2[i] = -1.0; }
  if (i < a.hd + a.hr) a.count[i] = 0;
  if (i == 0) {
    a.state[0] = 0; a.state[1] = 0; a.state[2] = (a.rows == 0 || a.M == 0) ? 1 : 0; a.state[3] = 0;
    a.counters[0] = 0; a.counters[1] = 0; a.counters[2] = 0; a.counters[3] = 0;
  }
}

// A thread per row: the box, the class; a narrow row is counted in the bucket of zhat's cell, a wide row joins the wide list.
__global__ __launch_bounds__(kGT) void assoc_grid_classify_kernel(const AssocGridArgs a) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.rows) return;
  const double* r = reinterpret_cast<const double*>(a.table + i);
  double reach2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { reach2[c] = assoc_grid_reach2(a.gate, a.sdiag[i * 3 + c]); a.reach2[i * 3 + c] = reach2[c]; }
  const int cls = assoc_grid_class(r[0], reach2, a.lim2);
  int bucket = -1;
  if (cls == kAssocGridNarrow) {
    bucket = (int)assoc_grid_hash(assoc_grid_coord(r[0], a.cell), assoc_grid_coord(r[1], a.cell), assoc_grid_coord(r[2], a.cell),
                                  (unsigned)(a.hr - 1));
    atomicAdd(&a.count[a.hd + bucket], 1);
  } else if (cls == kAssocGridWide) {
    a.wide[atomicAdd(&a.counters[0], 1)] = (int)i;
  }
  a.bucket_of[a.M + i] = bucket;
}

// A thread per detection: a finite position is counted in the bucket of its cell, any other is binned nowhere.
__global__ __launch_bounds__(kGT) void assoc_grid_bin_dets_kernel(const AssocGridArgs a) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.M) return;
  const double x = a.det[j * 7], y = a.det[j * 7 + 1], z = a.det[j * 7 + 2];
  int bucket = -1;
  if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0) {
    bucket = (int)assoc_grid_hash(assoc_grid_coord(x, a.cell), assoc_grid_coord(y, a.cell), assoc_grid_coord(z, a.cell), (unsigned)(a.hd - 1));
    atomicAdd(&a.count[bucket], 1);
  }
  a.bucket_of[j] = bucket;
}

// THE EXCLUSIVE SCAN of the counts, in three launches: per workgroup of kScanPerBlock counts the local exclusive prefix and the
// workgroup's sum; one workgroup scans the sums (with a carry, whatever their number) and writes the total behind the last start;
// then every start gets its workgroup's offset and the cursor its copy.
__device__ inline int block_exclusive_scan(int v, int* s, int tid, int* total) {
  s[tid] = v;
  __syncthreads();
  for (int o = 1; o < kGT; o <<= 1) {
    const int t = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  const int incl = s[tid];
  *total = s[kGT - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(kGT) void assoc_grid_scan_blocks_kernel(const AssocGridArgs a) {
  __shared__ int s[kGT];
  const long n = a.hd + a.hr;
  const int tid = (int)threadIdx.x;
  const long base = (long)blockIdx.x * kScanPerBlock + (long)tid * kScanPerThread;
  int v[kScanPerThread], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) { v[k] = base + k < n ? a.count[base + k] : 0; sum += v[k]; }
  int total;
  int run = block_exclusive_scan(sum, s, tid, &total);
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    if (base + k < n) a.start[base + k] = run;
    run += v[k];
  }
  if (tid == 0) a.sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kGT) void assoc_grid_scan_sums_kernel(const AssocGridArgs a, long n_blocks) {
  __shared__ int s[kGT];
  const int tid = (int)threadIdx.x;
  int carry = 0;
  for (long base = 0; base < n_blocks; base += kGT) {
    const int v = base + tid < n_blocks ? a.sums[base + tid] : 0;
    int total;
    const int excl = block_exclusive_scan(v, s, tid, &total);
    if (base + tid < n_blocks) a.sums[base + tid] = carry + excl;
    carry += total;
  }
  if (tid == 0) a.start[a.hd + a.hr] = carry;
}

__global__ __launch_bounds__(kGT) void assoc_grid_scan_add_kernel(const AssocGridArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.hd + a.hr) return;
  const int v = a.start[i] + a.sums[i / kScanPerBlock];
  a.start[i] = v;
  a.cursor[i] = v;
}

// A thread per detection and per row: into its bucket's stretch of the index list.  The order inside a stretch is the order the
// cursor's atomics happen to take; no output depends on it.
__global__ __launch_bounds__(kGT) void assoc_grid_place_kernel(const AssocGridArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.M + a.rows) return;
  const int b = a.bucket_of[i];
  if (b < 0) return;
  const bool is_det = i < a.M;
  const int pos = atomicAdd(&a.cursor[is_det ? (long)b : a.hd + b], 1);
  a.order[pos] = (int)(is_det ? i : i - a.M);
}

// the keyed minimum over the kWalkLanes lanes that share a walk: the key is total, so the order of the exchange does not matter
__device__ inline AssocBest walk_reduce(AssocBest best) {
#pragma unroll
  for (int o = kWalkLanes / 2; o > 0; o >>= 1) {
    const double d2 = __shfl_xor(best.d2, o, kWalkLanes);
    const int idx = __shfl_xor(best.idx, o, kWalkLanes);
    if (idx >= 0) assoc_take_keyed(best, d2, idx);
  }
  return best;
}

// TARGET-MAJOR, narrow rows.  kWalkLanes lanes own the t-th narrow row IN BUCKET ORDER -- the rows of a workgroup are rows of the
// same or of neighbouring buckets, so they read the same detections --, lane n < 27 walking the detection bucket of the n-th of the
// 27 cells around zhat's cell: 27 short dependent chains side by side instead of one long one.  A bucket met twice (a collision
// between two of the 27 cells) is walked twice: the keyed pick ignores repeats.
__global__ __launch_bounds__(kGT) void assoc_grid_scan_rows_kernel(const AssocGridArgs a) {
#pragma clang fp contract(off)
  if (a.state[2] != 0) return;   // (the whole grid reads the same word: settled by an earlier round)
  const int lane = (int)threadIdx.x % kWalkLanes;
  const long t = (long)blockIdx.x * kWalkPerWg + (int)threadIdx.x / kWalkLanes;
  const int first = a.start[a.hd];
  int row = -1;
  if (t < (long)(a.start[a.hd + a.hr] - first)) { row = a.order[first + t]; if (a.det_of_row[row] >= 0) row = -1; }
  AssocBest best = assoc_best_none();
  if (row >= 0 && lane < 27) {
    const double* r = reinterpret_cast<const double*>(a.table + row);
    double zh[3], W[6], reach2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { zh[c] = r[c]; reach2[c] = a.reach2[(long)row * 3 + c]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) W[k] = r[3 + k];
    const int cx = assoc_grid_coord(zh[0], a.cell), cy = assoc_grid_coord(zh[1], a.cell), cz = assoc_grid_coord(zh[2], a.cell);
    const unsigned b = assoc_grid_hash(cx + lane % 3 - 1, cy + (lane / 3) % 3 - 1, cz + lane / 9 - 1, (unsigned)(a.hd - 1));
    const int p1 = a.start[b + 1];
    for (int p = a.start[b]; p < p1; ++p) {
      const int j = a.order[p];
      if (a.row_of_det[j] >= 0) continue;
      double d2;
      if (assoc_grid_candidate(zh, W, reach2, a.det[(long)j * 7], a.det[(long)j * 7 + 1], a.det[(long)j * 7 + 2], a.gate, &d2))
        assoc_take_keyed(best, d2, j);
    }
  }
  best = walk_reduce(best);
  if (row >= 0 && lane == 0) { a.pick_row_d2[row] = best.d2; a.pick_row_idx[row] = best.idx; }
}

// TARGET-MAJOR, wide rows: a fixed grid strides over the wide list (its length is known on the device only); a thread owns a wide
// row and walks ALL detections, a tile at a time through LDS (a matched detection is staged as NaN), as assoc_scan_rows_kernel does.
__global__ __launch_bounds__(kGT) void assoc_grid_scan_wide_kernel(const AssocGridArgs a) {
#pragma clang fp contract(off)
  if (a.state[2] != 0) return;
  __shared__ double s_det[3][kGT];
  const int tid = (int)threadIdx.x;
  const long n_wide = a.counters[0];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (long wbase = (long)blockIdx.x * kGT; wbase < n_wide; wbase += (long)gridDim.x * kGT) {   // (uniform over the workgroup)
    const long w = wbase + tid;
    int row = -1;
    if (w < n_wide) { row = a.wide[w]; if (a.det_of_row[row] >= 0) row = -1; }
    double zh[3] = {0.0, 0.0, 0.0}, W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, reach2[3] = {0.0, 0.0, 0.0};
    if (row >= 0) {
      const double* r = reinterpret_cast<const double*>(a.table + row);
#pragma unroll
      for (int c = 0; c < 3; ++c) { zh[c] = r[c]; reach2[c] = a.reach2[(long)row * 3 + c]; }
#pragma unroll
      for (int k = 0; k < 6; ++k) W[k] = r[3 + k];
    }
    AssocBest best = assoc_best_none();
    for (long base = 0; base < a.M; base += kGT) {
      const long j = base + tid;
      double x = nan, y = nan, z = nan;
      if (j < a.M && a.row_of_det[j] < 0) { x = a.det[j * 7]; y = a.det[j * 7 + 1]; z = a.det[j * 7 + 2]; }
      __syncthreads();   // the tile before this one has been read
      s_det[0][tid] = x; s_det[1][tid] = y; s_det[2][tid] = z;
      __syncthreads();
      const int cnt = (int)((a.M - base) < (long)kGT ? (a.M - base) : (long)kGT);
      if (row >= 0) {
#pragma unroll 4
        for (int t = 0; t < cnt; ++t) {
          double d2;
          if (assoc_grid_candidate(zh, W, reach2, s_det[0][t], s_det[1][t], s_det[2][t], a.gate, &d2)) assoc_take_keyed(best, d2, (int)(base + t));
        }
      }
    }
    if (row >= 0) { a.pick_row_d2[row] = best.d2; a.pick_row_idx[row] = best.idx; }
  }
}

// DETECTION-MAJOR.  kWalkLanes lanes per detection: lane n < 27 walks the narrow rows in the row bucket of the n-th of the 27 cells
// around the detection's own cell (a narrow row that has this detection as a box-rule candidate lies there:
// associate_grid_plan.hpp); then every wide row, the wide list staged through LDS in tiles of kGT rows (a matched row's zhat[0]
// staged as NaN), the lanes of a detection striding over the tile.  A detection binned nowhere walks nothing and picks nothing.
__global__ __launch_bounds__(kGT) void assoc_grid_scan_dets_kernel(const AssocGridArgs a) {
#pragma clang fp contract(off)
  if (a.state[2] != 0) return;
  __shared__ double s_row[kGT * kWideWords];
  __shared__ int s_idx[kGT];
  const int tid = (int)threadIdx.x, lane = tid % kWalkLanes;
  const long j = (long)blockIdx.x * kWalkPerWg + tid / kWalkLanes;
  const bool open = j < a.M && a.row_of_det[j] < 0;
  const bool active = open && a.bucket_of[j] >= 0;
  double x = 0.0, y = 0.0, z = 0.0;
  AssocBest best = assoc_best_none();
  if (active) {
    x = a.det[j * 7]; y = a.det[j * 7 + 1]; z = a.det[j * 7 + 2];
    if (lane < 27) {
      const int cx = assoc_grid_coord(x, a.cell), cy = assoc_grid_coord(y, a.cell), cz = assoc_grid_coord(z, a.cell);
      const long g = a.hd + (long)assoc_grid_hash(cx + lane % 3 - 1, cy + (lane / 3) % 3 - 1, cz + lane / 9 - 1, (unsigned)(a.hr - 1));
      const int p1 = a.start[g + 1];
      for (int p = a.start[g]; p < p1; ++p) {
        const int row = a.order[p];
        if (a.det_of_row[row] >= 0) continue;
        const double* r = reinterpret_cast<const double*>(a.table + row);
        double d2;
        if (assoc_grid_candidate(r, r + 3, a.reach2 + (long)row * 3, x, y, z, a.gate, &d2)) assoc_take_keyed(best, d2, row);
      }
    }
  }
  const long n_wide = a.counters[0];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (long base = 0; base < n_wide; base += kGT) {   // (uniform over the workgroup)
    const int cnt = (int)((n_wide - base) < (long)kGT ? (n_wide - base) : (long)kGT);
    __syncthreads();   // the tile before this one has been read
    if (tid < cnt) {
      const int row = a.wide[base + tid];
      const double* r = reinterpret_cast<const double*>(a.table + row);
      double* s = s_row + tid * kWideWords;
#pragma unroll
      for (int k = 0; k < 9; ++k) s[k] = r[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) s[9 + c] = a.reach2[(long)row * 3 + c];
      if (a.det_of_row[row] >= 0) s[0] = nan;
      s_idx[tid] = row;
    }
    __syncthreads();
    if (active) {
      for (int t = lane; t < cnt; t += kWalkLanes) {
        const double* s = s_row + t * kWideWords;
        double d2;
        if (assoc_grid_candidate(s, s + 3, s + 9, x, y, z, a.gate, &d2)) assoc_take_keyed(best, d2, s_idx[t]);
      }
    }
  }
  best = walk_reduce(best);
  if (open && lane == 0) { a.pick_det_d2[j] = best.d2; a.pick_det_idx[j] = best.idx; }
}

// RESOLVE, over many workgroups: a thread per unmatched detection; if the row it picked picked it back, the two are matched -- one
// writer per word, since a row is picked back by one detection only.  d2_of_row is the target-major scan's value, d2_of_det the
// detection-major scan's.  The round's counts go through integer atomics, a pair per workgroup; assoc_grid_finish_kernel folds
// them into the state exactly as assoc_resolve_kernel does.
__global__ __launch_bounds__(kGT) void assoc_grid_resolve_kernel(const AssocGridArgs a) {
  if (a.state[2] != 0) return;
  __shared__ int s_matched[kGT / 64], s_open[kGT / 64];
  const int tid = (int)threadIdx.x;
  const long j = (long)blockIdx.x * kGT + tid;
  int matched = 0, open = 0;
  if (j < a.M && a.row_of_det[j] < 0) {
    const int i = a.pick_det_idx[j];
    if (i >= 0) {
      if (a.pick_row_idx[i] == (int)j) {
        a.row_of_det[j] = i; a.d2_of_det[j] = a.pick_det_d2[j];
        a.det_of_row[i] = (int)j; a.d2_of_row[i] = a.pick_row_d2[i];
        matched = 1;
      } else {
        open = 1;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { matched += __shfl_down(matched, o, 64); open += __shfl_down(open, o, 64); }
  if ((tid & 63) == 0) { s_matched[tid >> 6] = matched; s_open[tid >> 6] = open; }
  __syncthreads();
  if (tid == 0) {
    int m = 0, o = 0;
    for (int w = 0; w < kGT / 64; ++w) { m += s_matched[w]; o += s_open[w]; }
    if (m) atomicAdd(&a.counters[1], m);
    if (o) atomicAdd(&a.counters[2], o);
  }
}

__global__ void assoc_grid_finish_kernel(const AssocGridArgs a) {
  if (a.state[2] != 0) return;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  a.state[0] += a.counters[1];
  a.state[1] += 1;
  a.state[2] = a.counters[2] == 0 ? 1 : 0;
  a.counters[1] = 0; a.counters[2] = 0;
}

__global__ void assoc_grid_info_kernel(const int* counters, int* info) {
  if (blockIdx.x == 0 && threadIdx.x == 0) info[3] = counters[0];
}

// ---------------------------------------------------------------- the scratch (as AssocScratch::ensure: released before replaced)
void AssocScratch::ensure_grid(long rows, long dets, long buckets) {
  if (!grid_counters) grid_counters.alloc(4);
  if (rows > cap_grid_rows_ || !grid_wide) {
    const size_t want = rows > 64 ? rows : 64;
    cap_grid_rows_ = 0;
    grid_sdiag.alloc(want * 3); grid_reach2.alloc(want * 3); grid_wide.alloc(want);
    cap_grid_rows_ = (long)want;
  }
  if (rows + dets > cap_grid_dets_ || !grid_order) {
    const size_t want = rows + dets > 64 ? rows + dets : 64;
    cap_grid_dets_ = 0;
    grid_bucket_of.alloc(want); grid_order.alloc(want);
    cap_grid_dets_ = (long)want;
  }
  if (buckets > cap_grid_buckets_ || !grid_sums) {
    const size_t want = buckets > 64 ? buckets : 64;
    cap_grid_buckets_ = 0;
    grid_count.alloc(want); grid_start.alloc(want + 1); grid_cursor.alloc(want); grid_sums.alloc((want + kScanPerBlock - 1) / kScanPerBlock + 1);
    cap_grid_buckets_ = (long)want;
  }
}

// ---------------------------------------------------------------- the launches
namespace {
inline dim3 blocks_for(long n) { return dim3((unsigned)((n + kGT - 1) / kGT > 0 ? (n + kGT - 1) / kGT : 1)); }
inline dim3 walk_blocks_for(long n) { return dim3((unsigned)((n + kWalkPerWg - 1) / kWalkPerWg > 0 ? (n + kWalkPerWg - 1) / kWalkPerWg : 1)); }
}  // namespace

void launch_assoc_grid_match(const AssocScratch& s, long rows, const double* det, long M, double gate, double cell, int rounds,
                             const AssocGridBuckets& buckets, hipStream_t st) {
  AssocGridArgs a;
  a.table = s.table.get(); a.det = det; a.sdiag = s.grid_sdiag.get(); a.reach2 = s.grid_reach2.get();
  a.bucket_of = s.grid_bucket_of.get(); a.count = s.grid_count.get(); a.start = s.grid_start.get(); a.cursor = s.grid_cursor.get();
  a.sums = s.grid_sums.get(); a.order = s.grid_order.get(); a.wide = s.grid_wide.get(); a.counters = s.grid_counters.get();
  a.det_of_row = s.det_of_row.get(); a.d2_of_row = s.d2_of_row.get(); a.row_of_det = s.row_of_det.get(); a.d2_of_det = s.d2_of_det.get();
  a.pick_row_d2 = s.part_rows_d2.get(); a.pick_row_idx = s.part_rows_idx.get();
  a.pick_det_d2 = s.part_dets_d2.get(); a.pick_det_idx = s.part_dets_idx.get();
  a.state = s.state.get();
  a.rows = rows; a.M = M; a.hd = buckets.dets; a.hr = buckets.rows;
  a.gate = gate; a.cell = cell; a.lim2 = assoc_grid_narrow_limit2(cell);
  const long ht = buckets.total();
  long most = rows > M ? rows : M;
  if (ht > most) most = ht;
  const dim3 block(kGT);
  hipLaunchKernelGGL(assoc_grid_init_kernel, blocks_for(most), block, 0, st, a);
  if (rows > 0) hipLaunchKernelGGL(assoc_grid_classify_kernel, blocks_for(rows), block, 0, st, a);   // (info[3] also without detections)
  if (rows <= 0 || M <= 0) return;   // (the state says settled, no round run)
  hipLaunchKernelGGL(assoc_grid_bin_dets_kernel, blocks_for(M), block, 0, st, a);
  const long n_blocks = (ht + kScanPerBlock - 1) / kScanPerBlock;
  hipLaunchKernelGGL(assoc_grid_scan_blocks_kernel, dim3((unsigned)n_blocks), block, 0, st, a);
  hipLaunchKernelGGL(assoc_grid_scan_sums_kernel, dim3(1), block, 0, st, a, n_blocks);
  hipLaunchKernelGGL(assoc_grid_scan_add_kernel, blocks_for(ht), block, 0, st, a);
  hipLaunchKernelGGL(assoc_grid_place_kernel, blocks_for(M + rows), block, 0, st, a);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(assoc_grid_scan_rows_kernel, walk_blocks_for(rows), block, 0, st, a);
    hipLaunchKernelGGL(assoc_grid_scan_wide_kernel, dim3(kAssocGridWideWgs), block, 0, st, a);
    hipLaunchKernelGGL(assoc_grid_scan_dets_kernel, walk_blocks_for(M), block, 0, st, a);
    hipLaunchKernelGGL(assoc_grid_resolve_kernel, blocks_for(M), block, 0, st, a);
    hipLaunchKernelGGL(assoc_grid_finish_kernel, dim3(1), dim3(64), 0, st, a);
  }
}

long assoc_grid_scan_blocks(long buckets) { return (buckets + kScanPerBlock - 1) / kScanPerBlock; }

void launch_assoc_grid_bin_rows(const int* bucket_of, int* count, int* start, int* cursor, int* sums, int* order, long rows, long buckets,
                                hipStream_t st) {
  AssocGridArgs a{};   // (M = 0, hd = 0: the detection part of every array is empty, the kernels are the grid form's as they are)
  a.bucket_of = const_cast<int*>(bucket_of); a.count = count; a.start = start; a.cursor = cursor; a.sums = sums; a.order = order;
  a.rows = rows; a.M = 0; a.hd = 0; a.hr = buckets;
  const dim3 block(kGT);
  const long n_blocks = assoc_grid_scan_blocks(buckets);
  hipLaunchKernelGGL(assoc_grid_scan_blocks_kernel, dim3((unsigned)n_blocks), block, 0, st, a);
  hipLaunchKernelGGL(assoc_grid_scan_sums_kernel, dim3(1), block, 0, st, a, n_blocks);
  hipLaunchKernelGGL(assoc_grid_scan_add_kernel, blocks_for(buckets), block, 0, st, a);
  hipLaunchKernelGGL(assoc_grid_place_kernel, blocks_for(rows), block, 0, st, a);
}

void launch_assoc_grid_info(const AssocScratch& s, int* info, hipStream_t st) {
  if (!info) return;
  hipLaunchKernelGGL(assoc_grid_info_kernel, dim3(1), dim3(64), 0, st, s.grid_counters.get(), info);
}

}  // namespace te
