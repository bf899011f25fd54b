// select_soonest_plan.hpp -- no HIP: everything about "the k soonest sphere crossings" (target_batch_c.h,
// target_batch_select_soonest*) that is not a kernel -- the key and its order, the filler row, the argument checks, the split of
// the first stage's grid over the batches of a shard, and the merge of the shards' rows.  select_soonest.hip (the kernels),
// Shard / TargetManager (the host side) and tests/host/select_soonest_host_test.cpp (g++ alone) all build this header.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define TE_SOONEST_HD __host__ __device__
#else
#define TE_SOONEST_HD
#endif

namespace te {

constexpr int kSoonestMaxK = 256;          // TARGET_SOONEST_MAX_K: the rows of a result, and of every workgroup's list
constexpr int kSoonestChunk = 256;         // entries a workgroup looks at per round (= its threads)
constexpr int kSoonestFanIn = 32;          // lists a workgroup of the middle stage merges
constexpr int kSoonestMaxParts = 16;       // batches of one shard selected together (the parts travel as kernel arguments)
constexpr int kSoonestDefaultMaxWgs = 1024;   // first-stage workgroups unless TE_SELECT_SOONEST_MAX_WGS says otherwise
constexpr int kSoonestMaxWgsLimit = 4096;     // ... and the most the knob may ask for (the scratch is sized from it)

// THE KEY.  A candidate's delta is a non-negative, non-NaN double (delta_lo >= 0 is required), and the bits of such doubles order
// as unsigned integers once -0.0 has been folded into 0.0 (delta + 0.0).  Ties on delta break by batch index, then by slot: one
// 128-bit key, compared as (hi, lo).  No two candidates of a call have the same key, so the order is total and the result does not
// depend on the order in which candidates were collected.
struct SoonestKey {
  uint64_t hi;   // the canonical bits of delta
  uint64_t lo;   // batch << 32 | slot
};
// larger than every candidate's key (a candidate's hi is at most the bits of +inf): an empty row of a list
TE_SOONEST_HD inline SoonestKey soonest_key_none() { return SoonestKey{~0ull, ~0ull}; }
TE_SOONEST_HD inline bool soonest_key_is_none(const SoonestKey& a) { return a.hi == ~0ull; }
TE_SOONEST_HD inline bool soonest_key_less(const SoonestKey& a, const SoonestKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
TE_SOONEST_HD inline uint64_t soonest_delta_bits(double delta) {
  const double c = delta + 0.0;   // -0.0 -> 0.0; every other candidate value unchanged
  uint64_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = (uint64_t)__double_as_longlong(c);
#else
  std::memcpy(&u, &c, sizeof u);
#endif
  return u;
}
TE_SOONEST_HD inline SoonestKey soonest_key(double delta, int batch, int slot) {
  return SoonestKey{soonest_delta_bits(delta), ((uint64_t)(uint32_t)batch << 32) | (uint64_t)(uint32_t)slot};
}
TE_SOONEST_HD inline int soonest_key_batch(const SoonestKey& a) { return (int)(uint32_t)(a.lo >> 32); }
TE_SOONEST_HD inline int soonest_key_slot(const SoonestKey& a) { return (int)(uint32_t)(a.lo & 0xffffffffull); }
// THE CANDIDATE RULE, written as the contract writes it: a NaN delta fails both comparisons, -1 ("no intersection") fails the first
TE_SOONEST_HD inline bool soonest_candidate(double delta, bool ok, double lo, double hi) { return ok && delta >= lo && delta <= hi; }

// One row of a result as the host sees it.  The filler (rows count .. k-1) is what no_intersection (shard.hpp) writes.
struct SoonestRow {
  int batch = -1;
  int slot = -1;
  double delta = -1.0;
  double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
};
inline SoonestRow soonest_filler() { return SoonestRow{}; }
// the manager order on rows: (delta as doubles, so -0.0 == 0.0; batch; slot).  Rows handed in are candidates: no NaN.
inline bool soonest_row_less(const SoonestRow& a, const SoonestRow& b) {
  if (a.delta != b.delta) return a.delta < b.delta;
  if (a.batch != b.batch) return a.batch < b.batch;
  return a.slot < b.slot;
}

// THE REFUSALS that do not depend on a batch: k, the window, the output pairs.  Throws std::invalid_argument.
inline void check_soonest_window(long k, double delta_lo, double delta_hi) {
  const std::string pre = "target_estimation_amd: select_soonest: ";
  if (k < 1 || k > kSoonestMaxK) throw std::invalid_argument(pre + "k must be 1.." + std::to_string(kSoonestMaxK) + ", got " + std::to_string(k));
  if (!(delta_lo >= 0.0)) throw std::invalid_argument(pre + "delta_lo must be >= 0 (-1 is the library's \"no intersection\"), got " + std::to_string(delta_lo));
  if (!(delta_hi >= delta_lo)) throw std::invalid_argument(pre + "delta_hi must be >= delta_lo, got " + std::to_string(delta_hi));
}
// have_delta etc.: whether the pointer was given.  outputs_ok: every required output is there.
inline void check_soonest_args(long k, double delta_lo, double delta_hi, bool have_delta, bool have_pose, bool have_pose_out, bool outputs_ok) {
  const std::string pre = "target_estimation_amd: select_soonest: ";
  check_soonest_window(k, delta_lo, delta_hi);
  if (!have_delta) throw std::invalid_argument(pre + "delta is required");
  if (!outputs_ok) throw std::invalid_argument(pre + "every output but the pose rows is required");
  if (have_pose_out && !have_pose) throw std::invalid_argument(pre + "pose_out without pose: there is nothing to gather from");
  if (have_pose && !have_pose_out) throw std::invalid_argument(pre + "pose without pose_out: there is nowhere to gather to");
}

// THE FIRST STAGE'S GRID over the parts (batches) of one launch, split by cumulative workgroup counts as the population tick splits
// its parts.  chunks(n) = ceil(n / kSoonestChunk) rounds of work; a part gets one workgroup per chunk while the total stays within
// max_wgs, else its share of max_wgs (at least one while it has entries).  wg_begin[p] .. wg_begin[p + 1] are part p's workgroups;
// workgroup j of a part that has w of them takes chunks j, j + w, j + 2 w, ...: a trip count known when it starts.
// Returns the total (>= 1: an empty call still runs one workgroup, which writes an empty list).
inline int plan_soonest_grid(const long* n, int n_parts, int max_wgs, int* wg_begin /* [n_parts + 1] */) {
  if (max_wgs < 1) max_wgs = 1;
  long total_chunks = 0;
  for (int p = 0; p < n_parts; ++p) total_chunks += (n[p] + kSoonestChunk - 1) / kSoonestChunk;
  // a small call (up to two rounds each for one middle workgroup's lists) keeps to kSoonestFanIn workgroups: one middle workgroup then
  // merges them all and the last stage has a single list to pass on, which costs less than a second middle list would
  if (total_chunks <= 2 * kSoonestFanIn && max_wgs > kSoonestFanIn) max_wgs = kSoonestFanIn;
  int at = 0;
  for (int p = 0; p < n_parts; ++p) {
    const long c = (n[p] + kSoonestChunk - 1) / kSoonestChunk;
    long w = c;
    if (total_chunks > max_wgs) {
      w = (long)((double)max_wgs * (double)c / (double)total_chunks);
      if (w < 1 && c > 0) w = 1;
      if (w > c) w = c;
    }
    wg_begin[p] = at;
    at += (int)w;
  }
  wg_begin[n_parts] = at;
  return at > 0 ? at : 1;
}
// THE REFUSAL of a call with more batches of one device than a launch's arguments hold
inline void check_soonest_parts(long selected) {
  if (selected > kSoonestMaxParts)
    throw std::invalid_argument("target_estimation_amd: select_soonest: at most " + std::to_string(kSoonestMaxParts) + " batches of one device are selected together");
}
// workgroups of the middle stage for g first-stage lists
inline int soonest_mid_wgs(int g) { return (g + kSoonestFanIn - 1) / kSoonestFanIn; }
// rows of SoonestKey the scratch of one call holds for a first stage of g workgroups
inline size_t soonest_scratch_rows(int g) { return ((size_t)g + (size_t)soonest_mid_wgs(g)) * (size_t)kSoonestMaxK; }
// TE_SELECT_SOONEST_MAX_WGS as read from the environment (null or junk: the default), clamped to 1 .. kSoonestMaxWgsLimit
inline int soonest_max_wgs_from(const char* env) {
  if (!env || !env[0]) return kSoonestDefaultMaxWgs;
  char* end = nullptr;
  const long v = std::strtol(env, &end, 10);
  if (end == env) return kSoonestDefaultMaxWgs;
  return v < 1 ? 1 : v > kSoonestMaxWgsLimit ? kSoonestMaxWgsLimit : (int)v;
}

// THE MERGE of the shards' results: shard[s] holds count[s] <= k rows in the manager order, their batch indices already those of
// the whole manager.  out receives min(k, sum count) rows in that order and then fillers up to k; returns the count.
inline long merge_soonest(const std::vector<std::vector<SoonestRow>>& shard, long k, SoonestRow* out) {
  std::vector<size_t> at(shard.size(), 0);
  long n = 0;
  for (; n < k; ++n) {
    int best = -1;
    for (size_t s = 0; s < shard.size(); ++s) {
      if (at[s] >= shard[s].size()) continue;
      if (best < 0 || soonest_row_less(shard[s][at[s]], shard[(size_t)best][at[(size_t)best]])) best = (int)s;
    }
    if (best < 0) break;
    out[n] = shard[(size_t)best][at[(size_t)best]++];
  }
  for (long i = n; i < k; ++i) out[i] = soonest_filler();
  return n;
}

}  // namespace te
