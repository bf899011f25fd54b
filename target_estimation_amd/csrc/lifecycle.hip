// lifecycle.hip -- the kernels of the track lifecycle (lifecycle.hpp lists the launches; the rule is lifecycle_plan.hpp;
// DESIGN.md 3.20).  A unit of its own: no step kernel is touched.
#include "lifecycle.hpp"

#include "hip_check.hpp"

namespace te {

constexpr int kLT = kLifecycleThreads;

// A thread per slot: the counters behind this call go to the scratch (the batch's own are written by the commit only), the flag
// says stale.
__global__ __launch_bounds__(kLT) void lifecycle_count_kernel(const unsigned char* has, const unsigned char* miss, const unsigned char* hits,
                                                              unsigned char* new_miss, unsigned char* new_hits, unsigned char* flag, long n,
                                                              int max_misses) {
  const long i = (long)blockIdx.x * kLT + threadIdx.x;
  if (i >= n) return;
  const unsigned char seen = has[i];
  const unsigned char m = lifecycle_next_miss(seen, miss[i]), h = lifecycle_next_hits(seen, hits[i]);
  new_miss[i] = m; new_hits[i] = h;
  flag[i] = lifecycle_stale(max_misses, m) ? 1 : 0;
}

// A thread per detection.  The row is read only for an unmatched detection.
__global__ __launch_bounds__(kLT) void lifecycle_det_flag_kernel(const double* det, const int* slot_of_det, unsigned char* flag, long M) {
  const long j = (long)blockIdx.x * kLT + threadIdx.x;
  if (j >= M) return;
  const int slot = slot_of_det[j];
  unsigned char f = kLifecycleDetMatched;
  if (slot < 0) {
    double row[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) row[c] = det[j * 7 + c];
    f = lifecycle_det_flag(slot, row);
  }
  flag[j] = f;
}

// THE ORDERED COMPACTION.  The rank of a flagged entry inside its workgroup: the flagged lanes below it in its wavefront (ballot,
// popcount) plus the flagged entries of the wavefronts before its own (LDS); *block_total the workgroup's count.  Every thread of the
// workgroup calls it.
__device__ inline int block_rank(bool flagged, int tid, int* s_wave, int* block_total) {
  const unsigned long long ballot = __ballot(flagged);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) s_wave[wave] = __popcll(ballot);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kLifecycleWaves; ++w) { const int c = s_wave[w]; if (w < wave) before += c; total += c; }
  *block_total = total;
  return before + lifecycle_rank_in_wave(ballot, lane);
}

__global__ __launch_bounds__(kLT) void lifecycle_scan_blocks_kernel(const unsigned char* flag, unsigned char want, long n, int* sums) {
  __shared__ int s_wave[kLifecycleWaves];
  const int tid = (int)threadIdx.x;
  const long i = (long)blockIdx.x * kLT + tid;
  const bool flagged = i < n && flag[i] == want;
  int total;
  (void)block_rank(flagged, tid, s_wave, &total);
  if (tid == 0) sums[blockIdx.x] = total;
}

// One workgroup: the block counts become their exclusive prefix, a tile of kLT at a time with a carry; the total goes to *count_out.
__global__ __launch_bounds__(kLT) void lifecycle_scan_sums_kernel(int* sums, long n_blocks, int* count_out) {
  __shared__ int s[kLT];
  const int tid = (int)threadIdx.x;
  int carry = 0;
  for (long base = 0; base < n_blocks; base += kLT) {   // (uniform over the workgroup)
    const int v = base + tid < n_blocks ? sums[base + tid] : 0;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kLT; o <<= 1) {
      const int t = tid >= o ? s[tid - o] : 0;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    const int incl = s[tid], total = s[kLT - 1];
    __syncthreads();   // the tile has been read before the next one overwrites it
    if (base + tid < n_blocks) sums[base + tid] = carry + incl - v;
    carry += total;
  }
  if (tid == 0) *count_out = carry;
}

// Stage 3: position = the workgroup's offset + the rank inside it.  The position of a flagged entry is below the total, which is
// at most n: `list` needs room for n entries at most.
__global__ __launch_bounds__(kLT) void lifecycle_scatter_kernel(const unsigned char* flag, unsigned char want, long n, const int* sums, int* list) {
  __shared__ int s_wave[kLifecycleWaves];
  const int tid = (int)threadIdx.x;
  const long i = (long)blockIdx.x * kLT + tid;
  const bool flagged = i < n && flag[i] == want;
  int total;
  const int rank = block_rank(flagged, tid, s_wave, &total);
  if (flagged) {
    const long pos = (long)sums[blockIdx.x] + rank;
    if (pos < n) list[pos] = (int)i;
  }
}

__global__ __launch_bounds__(kLT) void lifecycle_commit_kernel(unsigned char* miss, unsigned char* hits, const unsigned char* new_miss,
                                                               const unsigned char* new_hits, long n) {
  const long i = (long)blockIdx.x * kLT + threadIdx.x;
  if (i < n) { miss[i] = new_miss[i]; hits[i] = new_hits[i]; }
}

__global__ __launch_bounds__(kLT) void lifecycle_moves_kernel(unsigned char* miss, unsigned char* hits, const int* src, const int* dst, long m) {
  const long i = (long)blockIdx.x * kLT + threadIdx.x;
  if (i < m) { miss[dst[i]] = miss[src[i]]; hits[dst[i]] = hits[src[i]]; }
}

// A thread per (row, word): consecutive threads store consecutive words of the staging.
__global__ __launch_bounds__(kLT) void lifecycle_gather_kernel(const double* det, const int* rows, long count, double* out) {
  const long t = (long)blockIdx.x * kLT + threadIdx.x;
  if (t >= count * 7) return;
  const long r = t / 7;
  const int c = (int)(t - r * 7);
  out[t] = det[(long)rows[r] * 7 + c];
}

// ---------------------------------------------------------------- the scratch (released before replaced: nothing is carried over)
void LifecycleScratch::ensure(long rows, long dets, long n_batches) {
  if (rows > cap_rows_ || !new_miss) {
    const size_t want = rows > 64 ? (size_t)rows : 64;
    cap_rows_ = -1;
    new_miss.alloc(want); new_hits.alloc(want);
    cap_rows_ = (long)want;
    cap_batches_ = -1;   // the pinned block holds the lists as well: sized below
  }
  if (rows + dets > cap_entries_ || !flag) {
    const size_t want = rows + dets > 64 ? (size_t)(rows + dets) : 64;
    cap_entries_ = -1;
    flag.alloc(want); list.alloc(want); sums.alloc((size_t)lifecycle_blocks((long)want) + 1);
    cap_entries_ = (long)want;
  }
  if (n_batches > cap_batches_ || !counts) {
    const size_t want = n_batches > 6 ? (size_t)n_batches : 6;
    cap_batches_ = -1;
    counts.alloc(want + 2);
    host.alloc(want + 2 + (size_t)cap_rows_);
    cap_batches_ = (long)want;
  }
}

// ---------------------------------------------------------------- the launches
namespace {
inline dim3 blocks_for(long n) { return dim3((unsigned)lifecycle_blocks(n)); }
}  // namespace

void launch_lifecycle_count(const unsigned char* has, const unsigned char* miss, const unsigned char* hits, unsigned char* new_miss,
                            unsigned char* new_hits, unsigned char* flag, long n, int max_misses, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lifecycle_count_kernel, blocks_for(n), dim3(kLT), 0, st, has, miss, hits, new_miss, new_hits, flag, n, max_misses);
  TE_HIP_CHECK(hipGetLastError());
}

void launch_lifecycle_det_flags(const double* det, const int* slot_of_det, unsigned char* flag, long M, hipStream_t st) {
  if (M <= 0) return;
  hipLaunchKernelGGL(lifecycle_det_flag_kernel, blocks_for(M), dim3(kLT), 0, st, det, slot_of_det, flag, M);
  TE_HIP_CHECK(hipGetLastError());
}

void launch_lifecycle_compact(const unsigned char* flag, unsigned char want, long n, int* sums, int* list, int* count_out, hipStream_t st) {
  const long n_blocks = n > 0 ? lifecycle_blocks(n) : 0;   // (n == 0: the sums kernel alone writes the zero count)
  if (n_blocks > 0) hipLaunchKernelGGL(lifecycle_scan_blocks_kernel, dim3((unsigned)n_blocks), dim3(kLT), 0, st, flag, want, n, sums);
  hipLaunchKernelGGL(lifecycle_scan_sums_kernel, dim3(1), dim3(kLT), 0, st, sums, n_blocks, count_out);
  if (n_blocks > 0 && list) hipLaunchKernelGGL(lifecycle_scatter_kernel, dim3((unsigned)n_blocks), dim3(kLT), 0, st, flag, want, n, sums, list);
  TE_HIP_CHECK(hipGetLastError());
}

void launch_lifecycle_commit(unsigned char* miss, unsigned char* hits, const unsigned char* new_miss, const unsigned char* new_hits, long n,
                             hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lifecycle_commit_kernel, blocks_for(n), dim3(kLT), 0, st, miss, hits, new_miss, new_hits, n);
  TE_HIP_CHECK(hipGetLastError());
}

void launch_lifecycle_moves(unsigned char* miss, unsigned char* hits, const int* src, const int* dst, long m, hipStream_t st) {
  if (m <= 0) return;
  hipLaunchKernelGGL(lifecycle_moves_kernel, blocks_for(m), dim3(kLT), 0, st, miss, hits, src, dst, m);
  TE_HIP_CHECK(hipGetLastError());
}

void launch_lifecycle_gather(const double* det, const int* rows, long count, double* out, hipStream_t st) {
  if (count <= 0) return;
  hipLaunchKernelGGL(lifecycle_gather_kernel, blocks_for(count * 7), dim3(kLT), 0, st, det, rows, count, out);
  TE_HIP_CHECK(hipGetLastError());
}

}  // namespace te
