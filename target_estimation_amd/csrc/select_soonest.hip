// select_soonest.hip -- the kernels of select_soonest.hpp and their launches.  One kernel family whatever the batches' model,
// precision and layout: the query's outputs are doubles.
#include "select_soonest.hpp"

#include "hip_check.hpp"

namespace te {

namespace {

constexpr int kThreads = kSoonestChunk;        // 4 wavefronts
constexpr int kWaves = kThreads / 64;
constexpr int kList = 2 * kSoonestMaxK;        // keys of a workgroup's list: [0, 256) the best so far, [256, 512) collected
static_assert(kThreads == kSoonestMaxK, "one thread per row of a list");

// everything both kernels read, by value (no table in device memory: nothing to upload, nothing a captured graph could outlive)
struct SoonestArgs {
  SoonestPart part[kSoonestMaxParts];
  int wg_begin[kSoonestMaxParts + 1];   // scan: part p owns workgroups wg_begin[p] .. wg_begin[p + 1]
  int n_parts;
  int k;
  double lo, hi;
  const SoonestKey* in;   // merge: n_lists lists of k rows each; workgroup w merges lists w * fan .. min(n_lists, (w + 1) * fan)
  int n_lists;
  int fan;
  SoonestKey* lists;      // scan and the middle merge: where workgroup w writes its k rows (lists + w * k)
  SoonestOut out;         // the last merge (out.slot != null): the result
};

// ---- a workgroup's list in LDS
__device__ inline void list_init(SoonestKey* s) {
  s[threadIdx.x] = soonest_key_none();
  s[threadIdx.x + kSoonestMaxK] = soonest_key_none();
  __syncthreads();
}

// ascending bitonic sort of the kList keys, one compare-exchange per thread and step (45 steps)
__device__ inline void list_sort(SoonestKey* s) {
  const int t = (int)threadIdx.x;
#pragma unroll 1
  for (int size = 2; size <= kList; size <<= 1) {
#pragma unroll 1
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int i = 2 * t - (t & (stride - 1));
      const int j = i + stride;
      const bool asc = (i & size) == 0;
      const SoonestKey a = s[i], b = s[j];
      if (soonest_key_less(b, a) == asc) { s[i] = b; s[j] = a; }
    }
  }
  __syncthreads();
}

// One round: the threads whose `keep` is set put `key` behind the keys collected so far, in thread order.  Until the first sort the
// whole list collects (start 0: 512 places); from then on its upper half does (start 256), the lower half holding the best so far,
// sorted.  When a round's keys do not fit, the list is sorted first (the best kSoonestMaxK stay, the rest is dropped), and `thr`
// becomes the k-th best key: no key at or above it can be among the k best of anything that contains this list.  start, fill and
// thr are uniform over the workgroup.
__device__ inline void list_add(SoonestKey* s, int* s_wave, bool keep, const SoonestKey& key, int k, int& start, int& fill, SoonestKey& thr) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const unsigned long long votes = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(votes);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = s_wave[w];
    if (w < wave) base += c;
    total += c;
  }
  if (total > 0) {   // uniform
    if (start + fill + total > kList) {
      list_sort(s);
      thr = s[k - 1];
      s[threadIdx.x + kSoonestMaxK] = soonest_key_none();
      start = kSoonestMaxK;
      fill = 0;
      __syncthreads();   // the collecting half is empty before anyone puts a key there
    }
    if (keep) s[start + fill + base + __popcll(votes & ((1ull << lane) - 1ull))] = key;
    fill += total;
  }
  __syncthreads();   // s_wave is rewritten by the next round
}

}  // namespace

// Stage 1.  Workgroup j of a part that has w workgroups looks at chunks j, j + w, ... of the part's arrays.
__global__ __launch_bounds__(kThreads) void soonest_scan_kernel(const SoonestArgs a) {
  __shared__ SoonestKey s[kList];
  __shared__ int s_wave[kWaves];
  const int wg = (int)blockIdx.x, t = (int)threadIdx.x;
  list_init(s);
  const double* delta = nullptr;
  const unsigned char* okp = nullptr;
  long n = 0;
  int batch = 0, first = 0, w = 1;
#pragma unroll
  for (int p = 0; p < kSoonestMaxParts; ++p)
    if (p < a.n_parts && wg >= a.wg_begin[p] && wg < a.wg_begin[p + 1]) {
      delta = a.part[p].delta; okp = a.part[p].ok; n = a.part[p].n; batch = a.part[p].batch;
      first = a.wg_begin[p]; w = a.wg_begin[p + 1] - a.wg_begin[p];
    }
  const long chunks = (n + kSoonestChunk - 1) / kSoonestChunk;
  const long j = wg - first;
  const long rounds = j < chunks ? (chunks - j + w - 1) / w : 0;
  int start = 0, fill = 0;
  SoonestKey thr = soonest_key_none();
  for (long r = 0; r < rounds; ++r) {
    const long i = (j + r * w) * kSoonestChunk + t;
    bool keep = false;
    SoonestKey key = soonest_key_none();
    if (i < n) {
      const double d = delta[i];
      const bool ok = okp == nullptr || okp[i] != 0;
      if (soonest_candidate(d, ok, a.lo, a.hi)) {
        key = soonest_key(d, batch, (int)i);
        keep = soonest_key_less(key, thr);
      }
    }
    list_add(s, s_wave, keep, key, a.k, start, fill, thr);
  }
  if (fill > 0) list_sort(s);   // (nothing collected since the last sort, or nothing at all: the list is in order as it is)
  if (t < a.k) a.lists[(long)wg * a.k + t] = s[t];
}

// Stages 2 and 3.  With a.out.slot set (one workgroup) the k rows are the result: slot, batch, delta as the input's own bits, pose.
__global__ __launch_bounds__(kThreads) void soonest_merge_kernel(const SoonestArgs a) {
  __shared__ SoonestKey s[kList];
  __shared__ int s_wave[kWaves];
  const int wg = (int)blockIdx.x, t = (int)threadIdx.x;
  list_init(s);
  const long first = (long)wg * a.fan;
  const long lists = first < a.n_lists ? (a.n_lists - first < a.fan ? a.n_lists - first : a.fan) : 0;
  const long rows = lists * a.k;
  const long rounds = (rows + kThreads - 1) / kThreads;
  const SoonestKey* in = a.in + first * a.k;
  int start = 0, fill = 0;
  SoonestKey thr = soonest_key_none();
  for (long r = 0; r < rounds; ++r) {
    const long i = r * kThreads + t;
    SoonestKey key = soonest_key_none();
    if (i < rows) key = in[i];
    const bool keep = !soonest_key_is_none(key) && soonest_key_less(key, thr);
    list_add(s, s_wave, keep, key, a.k, start, fill, thr);
  }
  // (one list alone was placed in thread order, which is its own order: the last stage behind a single middle workgroup sorts nothing)
  if (fill > 0 && lists != 1) list_sort(s);
  if (t >= a.k) return;
  const SoonestKey key = s[t];
  if (a.out.slot == nullptr) {
    a.lists[(long)wg * a.k + t] = key;
    return;
  }
  const bool valid = !soonest_key_is_none(key);
  int batch = -1, slot = -1;
  double d = -1.0;
  double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  if (valid) {
    batch = soonest_key_batch(key);
    slot = soonest_key_slot(key);
    const double* delta = nullptr;
    const double* posep = nullptr;
#pragma unroll
    for (int p = 0; p < kSoonestMaxParts; ++p)
      if (p < a.n_parts && a.part[p].batch == batch) { delta = a.part[p].delta; posep = a.part[p].pose; }
    d = delta[slot];
    if (a.out.pose != nullptr && posep != nullptr) {
#pragma unroll
      for (int c = 0; c < 7; ++c) pose[c] = posep[(long)slot * 7 + c];
    }
  }
  a.out.slot[t] = slot;
  if (a.out.batch != nullptr) a.out.batch[t] = batch;
  a.out.delta[t] = d;
  if (a.out.pose != nullptr) {
#pragma unroll
    for (int c = 0; c < 7; ++c) a.out.pose[t * 7 + c] = pose[c];
  }
  // the valid rows are a prefix of the sorted list: the thread at its end says how long it is
  if (valid ? (t == a.k - 1 || soonest_key_is_none(s[t + 1])) : t == 0) a.out.count[0] = valid ? t + 1 : 0;
}

// ---------------------------------------------------------------- host side
void SoonestScratch::ensure(int max_wgs) {
  if (result_host_) return;   // (allocated last: its presence stands for all three)
  max_wgs_ = max_wgs < 1 ? 1 : max_wgs > kSoonestMaxWgsLimit ? kSoonestMaxWgsLimit : max_wgs;
  // (a part with entries gets at least one workgroup: the grid may exceed the knob by the number of parts)
  lists_.alloc(soonest_scratch_rows(max_wgs_ + kSoonestMaxParts));
  result_dev_.alloc(kResultBytes);
  result_host_.alloc(kResultBytes);
}

SoonestOut SoonestScratch::result_out(bool with_pose) const {
  char* d = result_dev_.get();
  return SoonestOut{(int*)(d + kOffBatch), (int*)(d + kOffSlot), (double*)(d + kOffDelta), with_pose ? (double*)(d + kOffPose) : nullptr,
                    (int*)(d + kOffCount)};
}

void launch_select_soonest(const SoonestPart* parts, int n_parts, double delta_lo, double delta_hi, int k, const SoonestOut& out,
                           const SoonestScratch& scratch, hipStream_t st) {
  if (n_parts < 0 || n_parts > kSoonestMaxParts)
    throw std::invalid_argument("target_estimation_amd: select_soonest: at most " + std::to_string(kSoonestMaxParts) + " batches of one device are selected together");
  if (!scratch.lists()) throw std::logic_error("target_estimation_amd: select_soonest: the scratch has not been allocated");
  SoonestArgs a{};
  long n[kSoonestMaxParts];
  for (int p = 0; p < n_parts; ++p) { a.part[p] = parts[p]; n[p] = parts[p].n; }
  const int g = plan_soonest_grid(n, n_parts, scratch.max_wgs(), a.wg_begin);
  for (int p = n_parts + 1; p <= kSoonestMaxParts; ++p) a.wg_begin[p] = a.wg_begin[n_parts];
  const int g2 = soonest_mid_wgs(g);
  a.n_parts = n_parts; a.k = k; a.lo = delta_lo; a.hi = delta_hi;
  SoonestKey* lists1 = scratch.lists();
  SoonestKey* lists2 = lists1 + (size_t)g * (size_t)k;
  a.lists = lists1;
  hipLaunchKernelGGL(soonest_scan_kernel, dim3((unsigned)g), dim3(kThreads), 0, st, a);
  a.in = lists1; a.n_lists = g; a.fan = kSoonestFanIn; a.lists = lists2;
  hipLaunchKernelGGL(soonest_merge_kernel, dim3((unsigned)g2), dim3(kThreads), 0, st, a);
  a.in = lists2; a.n_lists = g2; a.fan = g2; a.lists = nullptr; a.out = out;
  hipLaunchKernelGGL(soonest_merge_kernel, dim3(1), dim3(kThreads), 0, st, a);
  TE_HIP_CHECK(hipGetLastError());
}

long select_soonest_to_host(const SoonestPart* parts, int n_parts, double delta_lo, double delta_hi, int k, bool with_pose,
                            SoonestScratch& scratch, hipStream_t st, SoonestRow* rows) {
  select_soonest_begin(parts, n_parts, delta_lo, delta_hi, k, with_pose, scratch, st);
  return select_soonest_end(k, with_pose, scratch, st, rows);
}

void select_soonest_begin(const SoonestPart* parts, int n_parts, double delta_lo, double delta_hi, int k, bool with_pose,
                          SoonestScratch& scratch, hipStream_t st) {
  launch_select_soonest(parts, n_parts, delta_lo, delta_hi, k, scratch.result_out(with_pose), scratch, st);
  TE_HIP_CHECK(hipMemcpyAsync(scratch.result_host(), scratch.result_dev(), SoonestScratch::kResultBytes, hipMemcpyDeviceToHost, st));
}

long select_soonest_end(int k, bool with_pose, SoonestScratch& scratch, hipStream_t st, SoonestRow* rows) {
  TE_HIP_CHECK(hipStreamSynchronize(st));
  const char* h = scratch.result_host();
  const int* hb = (const int*)(h + SoonestScratch::kOffBatch);
  const int* hs = (const int*)(h + SoonestScratch::kOffSlot);
  const double* hd = (const double*)(h + SoonestScratch::kOffDelta);
  const double* hp = (const double*)(h + SoonestScratch::kOffPose);
  const long count = *(const int*)(h + SoonestScratch::kOffCount);
  for (int i = 0; i < k; ++i) {
    rows[i] = soonest_filler();
    if (i >= count) continue;
    rows[i].batch = hb[i]; rows[i].slot = hs[i]; rows[i].delta = hd[i];
    if (with_pose) for (int c = 0; c < 7; ++c) rows[i].pose[c] = hp[i * 7 + c];
  }
  return count;
}

}  // namespace te
