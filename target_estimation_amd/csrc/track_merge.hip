// track_merge.hip -- the kernels of the duplicate-track search (track_merge.hpp lists the launches; the rule is
// track_merge_plan.hpp).  A unit of its own: the table kernel is the association's (associate.hip), the scan and
// the placement are the grid form's (associate_grid.hip), neither is changed.
#include "track_merge.hpp"

#include "associate_grid.hpp"
#include "hip_check.hpp"

namespace te {

constexpr int kMT = kMergeThreads;
constexpr int kMergeWalkLanes = 32;                 // lanes that share ONE row's walk: a lane per cell of the 27, five idle
constexpr int kMergeWalkPerWg = kMT / kMergeWalkLanes;

struct MergeArgs {
  const AssocRow* table;   // MergeRows
  unsigned char* hits;     // [rows]
  unsigned char* miss;
  int* bucket_of;
  int* order;              // the eligible rows grouped by bucket
  int* count;              // [h]
  const int* start;        // [h + 1]
  int* partner;
  int* pick_idx;
  double* d2;
  double* pick_d2;
  int* state;
  int* counters;
  long rows, h;
  double gate, cell, lim2;
  int min_hits;
};

__global__ __launch_bounds__(kMT) void merge_init_kernel(const MergeArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.rows) { a.partner[i] = -1; a.d2[i] = -1.0; a.pick_idx[i] = -1; a.pick_d2[i] = -1.0; }
  if (i < a.h) a.count[i] = 0;
  if (i == 0) {
    a.state[0] = 0; a.state[1] = 0; a.state[2] = a.rows == 0 ? 1 : 0; a.state[3] = 0;
    a.counters[0] = 0; a.counters[1] = 0; a.counters[2] = 0; a.counters[3] = 0;
  }
}

// A thread per slot of one batch: the class; an eligible row is counted in the bucket of its cell, a wide row in counters[0].
__global__ __launch_bounds__(kMT) void merge_classify_kernel(const MergeArgs a, long row_offset, long size, const unsigned char* hits,
                                                             const unsigned char* miss) {
#pragma clang fp contract(off)
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= size) return;
  const long i = row_offset + slot;
  const double* r = reinterpret_cast<const double*>(a.table + i);
  double row[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) row[k] = r[k];
  const unsigned char h = hits[slot];
  a.hits[i] = h;
  a.miss[i] = miss[slot];
  const int cls = merge_row_class(row, (int)h, a.min_hits, a.gate, a.lim2);
  int bucket = -1;
  if (cls == kMergeEligible) {
    bucket = (int)assoc_grid_hash(assoc_grid_coord(row[0], a.cell), assoc_grid_coord(row[1], a.cell), assoc_grid_coord(row[2], a.cell),
                                  (unsigned)(a.h - 1));
    atomicAdd(&a.count[bucket], 1);
  } else if (cls == kMergeWide) {
    atomicAdd(&a.counters[0], 1);
  }
  a.bucket_of[i] = bucket;
}

// the keyed minimum over the lanes that share a walk: the key is total, so the order of the exchange does not matter
__device__ inline AssocBest merge_walk_reduce(AssocBest best) {
#pragma unroll
  for (int o = kMergeWalkLanes / 2; o > 0; o >>= 1) {
    const double d2 = __shfl_xor(best.d2, o, kMergeWalkLanes);
    const int idx = __shfl_xor(best.idx, o, kMergeWalkLanes);
    if (idx >= 0) assoc_take_keyed(best, d2, idx);
  }
  return best;
}

// THE SELF-SCAN.  kMergeWalkLanes lanes own the t-th eligible row IN BUCKET ORDER -- the rows of a workgroup are rows of the same
// or of neighbouring buckets, so they read the same rows --, lane n < 27 walking the row bucket of the n-th of the 27 cells around
// the row's own cell.  A visit is one 80-byte record: the pair (lo, hi) is ordered by row index with selects, so that both partners
// form the same C, V and d2.  A bucket met twice is walked twice: the keyed pick ignores repeats; a row never picks itself.
__global__ __launch_bounds__(kMT) void merge_scan_kernel(const MergeArgs a) {
#pragma clang fp contract(off)
  if (a.state[2] != 0) return;   // (the whole grid reads the same word: settled by an earlier round)
  const int lane = (int)threadIdx.x % kMergeWalkLanes;
  const long t = (long)blockIdx.x * kMergeWalkPerWg + (int)threadIdx.x / kMergeWalkLanes;
  int row = -1;
  if (t < (long)a.start[a.h]) { row = a.order[t]; if (a.partner[row] >= 0) row = -1; }
  AssocBest best = assoc_best_none();
  if (row >= 0 && lane < 27) {
    const double* rows = reinterpret_cast<const double*>(a.table);
    double me[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) me[k] = rows[(long)row * kAssocRowWords + k];
    const int cx = assoc_grid_coord(me[0], a.cell), cy = assoc_grid_coord(me[1], a.cell), cz = assoc_grid_coord(me[2], a.cell);
    const unsigned b = assoc_grid_hash(cx + lane % 3 - 1, cy + (lane / 3) % 3 - 1, cz + lane / 9 - 1, (unsigned)(a.h - 1));
    const int p1 = a.start[b + 1];
    for (int p = a.start[b]; p < p1; ++p) {
      const int j = a.order[p];
      if (j == row || a.partner[j] >= 0) continue;
      double lo[9], hi[9];
      const bool first = row < j;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double o = rows[(long)j * kAssocRowWords + k];
        lo[k] = first ? me[k] : o;
        hi[k] = first ? o : me[k];
      }
      double d2;
      if (merge_pair_candidate(lo, hi, a.gate, &d2)) assoc_take_keyed(best, d2, j);
    }
  }
  best = merge_walk_reduce(best);
  if (row >= 0 && lane == 0) { a.pick_d2[row] = best.d2; a.pick_idx[row] = best.idx; }
}

// RESOLVE, over many workgroups: a thread per unmatched row that picked; if the row it picked picked it back, the two are a pair.
// Each of the two threads writes ITS OWN partner and d2 (the same bits: the pair is ordered (lo, hi) on both sides), so every word
// has one writer; the picks are read only.  The lower row counts the pair.
__global__ __launch_bounds__(kMT) void merge_resolve_kernel(const MergeArgs a) {
  if (a.state[2] != 0) return;
  __shared__ int s_matched[kMT / 64], s_open[kMT / 64];
  const int tid = (int)threadIdx.x;
  const long i = (long)blockIdx.x * kMT + tid;
  int matched = 0, open = 0;
  if (i < a.rows && a.partner[i] < 0) {
    const int j = a.pick_idx[i];
    if (j >= 0) {
      if (a.pick_idx[j] == (int)i) {
        a.partner[i] = j; a.d2[i] = a.pick_d2[i];
        if (i < (long)j) matched = 1;
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
    for (int w = 0; w < kMT / 64; ++w) { m += s_matched[w]; o += s_open[w]; }
    if (m) atomicAdd(&a.counters[1], m);
    if (o) atomicAdd(&a.counters[2], o);
  }
}

__global__ void merge_finish_kernel(const MergeArgs a) {
  if (a.state[2] != 0) return;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  a.state[0] += a.counters[1];
  a.state[1] += 1;
  a.state[2] = a.counters[2] == 0 ? 1 : 0;
  a.counters[1] = 0; a.counters[2] = 0;
}

// A thread per slot of one batch: the weaker row of a pair is the duplicate; the partner's tag gives (batch, slot).
__global__ __launch_bounds__(kMT) void merge_out_kernel(const AssocRow* table, const int* partner, const double* d2, const unsigned char* hits,
                                                        const unsigned char* miss, long row_offset, long size, unsigned char* dup,
                                                        int* partner_batch, int* partner_slot, double* d2_of_slot) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= size) return;
  const long i = row_offset + slot;
  const int j = partner[i];
  int pb = -1, ps = -1;
  bool weaker = false;
  if (j >= 0) {
    const long long tag = reinterpret_cast<const long long*>(table + j)[9];
    ps = (int)(unsigned)(tag & 0xffffffffll);
    pb = (int)(tag >> 32);
    weaker = merge_is_weaker((int)hits[i], (int)miss[i], (int)i, (int)hits[j], (int)miss[j], j);
  }
  dup[slot] = weaker ? 1 : 0;
  if (partner_batch) partner_batch[slot] = pb;
  if (partner_slot) partner_slot[slot] = ps;
  if (d2_of_slot) d2_of_slot[slot] = j >= 0 ? d2[i] : -1.0;
}

__global__ void merge_info_kernel(const int* state, const int* counters, int* info) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { info[0] = state[0]; info[1] = state[1]; info[2] = state[2]; info[3] = counters[0]; }
}

__global__ __launch_bounds__(kMT) void merge_gather_kernel(const int* list, const int* count, long size, const int* partner_batch,
                                                           const int* partner_slot, int* list_batch, int* list_slot) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= size || k >= (long)*count) return;
  const int slot = list[k];
  list_batch[k] = partner_batch[slot];
  list_slot[k] = partner_slot[slot];
}

// ---------------------------------------------------------------- the scratch (released before replaced: nothing is carried over)
void MergeScratch::ensure(long rows, long buckets) {
  if (!counters) { state.alloc(4); counters.alloc(4); }
  if (rows > cap_rows_ || !pick_d2) {
    const size_t want = rows > 64 ? (size_t)rows : 64;
    cap_rows_ = -1;
    table.alloc(want); hits.alloc(want); miss.alloc(want); bucket_of.alloc(want); order.alloc(want);
    partner.alloc(want); pick_idx.alloc(want); d2.alloc(want); pick_d2.alloc(want);
    cap_rows_ = (long)want;
  }
  if (buckets > cap_buckets_ || !sums) {
    const size_t want = buckets > 64 ? (size_t)buckets : 64;
    cap_buckets_ = -1;
    count.alloc(want); start.alloc(want + 1); cursor.alloc(want); sums.alloc((size_t)assoc_grid_scan_blocks((long)want) + 1);
    cap_buckets_ = (long)want;
  }
}

void MergeScratch::ensure_retire(long rows, long n_batches) {
  const bool grow_rows = rows > cap_retire_rows_ || !csums;
  const bool grow_batches = n_batches > cap_retire_batches_ || !counts;
  if (grow_rows) {
    const size_t want = rows > 64 ? (size_t)rows : 64;
    cap_retire_rows_ = -1;
    dup.alloc(want); partner_batch.alloc(want); partner_slot.alloc(want); list.alloc(want); list_batch.alloc(want); list_slot.alloc(want);
    csums.alloc((size_t)((want + kMT - 1) / kMT) + 1);
    cap_retire_rows_ = (long)want;
  }
  if (grow_batches) {
    const size_t want = n_batches > 6 ? (size_t)n_batches : 6;
    cap_retire_batches_ = -1;
    counts.alloc(want + 4);
    cap_retire_batches_ = (long)want;
  }
  if (grow_rows || grow_batches || !host) host.alloc((size_t)cap_retire_batches_ + 4 + 3 * (size_t)cap_retire_rows_);
}

// ---------------------------------------------------------------- the launches
namespace {
inline dim3 blocks_for(long n) { return dim3((unsigned)((n + kMT - 1) / kMT > 0 ? (n + kMT - 1) / kMT : 1)); }
inline dim3 walk_blocks_for(long n) { return dim3((unsigned)((n + kMergeWalkPerWg - 1) / kMergeWalkPerWg > 0 ? (n + kMergeWalkPerWg - 1) / kMergeWalkPerWg : 1)); }
}  // namespace

void launch_merge_match(const MergeScratch& s, long rows, const MergeBatchIn* in, int n_batches, double gate, double cell, int rounds,
                        int min_hits, long buckets, hipStream_t st) {
  MergeArgs a;
  a.table = s.table.get(); a.hits = s.hits.get(); a.miss = s.miss.get(); a.bucket_of = s.bucket_of.get(); a.order = s.order.get();
  a.count = s.count.get(); a.start = s.start.get(); a.partner = s.partner.get(); a.pick_idx = s.pick_idx.get(); a.d2 = s.d2.get();
  a.pick_d2 = s.pick_d2.get(); a.state = s.state.get(); a.counters = s.counters.get();
  a.rows = rows; a.h = buckets; a.gate = gate; a.cell = cell; a.lim2 = assoc_grid_narrow_limit2(cell); a.min_hits = min_hits;
  const dim3 block(kMT);
  hipLaunchKernelGGL(merge_init_kernel, blocks_for(rows > buckets ? rows : buckets), block, 0, st, a);
  if (rows <= 0) return;   // (the state says settled, no round run)
  long off = 0;
  for (int b = 0; b < n_batches; ++b) {
    if (in[b].size > 0) hipLaunchKernelGGL(merge_classify_kernel, blocks_for(in[b].size), block, 0, st, a, off, in[b].size, in[b].hits, in[b].miss);
    off += in[b].size;
  }
  launch_assoc_grid_bin_rows(s.bucket_of.get(), s.count.get(), s.start.get(), s.cursor.get(), s.sums.get(), s.order.get(), rows, buckets, st);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(merge_scan_kernel, walk_blocks_for(rows), block, 0, st, a);
    hipLaunchKernelGGL(merge_resolve_kernel, blocks_for(rows), block, 0, st, a);
    hipLaunchKernelGGL(merge_finish_kernel, dim3(1), dim3(64), 0, st, a);
  }
}

void launch_merge_out(const MergeScratch& s, long row_offset, long size, const MergeSlotOut& out, hipStream_t st) {
  if (size <= 0) return;
  hipLaunchKernelGGL(merge_out_kernel, blocks_for(size), dim3(kMT), 0, st, s.table.get(), s.partner.get(), s.d2.get(), s.hits.get(), s.miss.get(),
                     row_offset, size, out.dup, out.partner_batch, out.partner_slot, out.d2);
}

void launch_merge_info(const MergeScratch& s, int* info, hipStream_t st) {
  hipLaunchKernelGGL(merge_info_kernel, dim3(1), dim3(64), 0, st, s.state.get(), s.counters.get(), info);
}

void launch_merge_gather(const MergeScratch& s, long row_offset, long size, const int* count_dev, hipStream_t st) {
  if (size <= 0) return;
  hipLaunchKernelGGL(merge_gather_kernel, blocks_for(size), dim3(kMT), 0, st, s.list.get() + row_offset, count_dev, size,
                     s.partner_batch.get() + row_offset, s.partner_slot.get() + row_offset, s.list_batch.get() + row_offset,
                     s.list_slot.get() + row_offset);
}

}  // namespace te
