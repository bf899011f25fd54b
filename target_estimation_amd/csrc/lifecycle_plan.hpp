// lifecycle_plan.hpp -- no HIP: everything about the track lifecycle (target_batch_c.h, target_manager_lifecycle)
// that is not a kernel -- the per-slot counters, the stale and born rules, the block arithmetic of the ordered compaction, the
// refusals that need no handle, the id-range check.  lifecycle.hip (the kernels), Shard / TargetManager (the host side) and
// tests/host/lifecycle_plan_host_test.cpp (g++ alone) all build this header.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>

#if defined(__HIPCC__)
#define TE_LC_HD __host__ __device__
#else
#define TE_LC_HD
#endif

namespace te {

constexpr long kLifecycleMaxDetections = 1048576;   // TARGET_ASSOC_GRID_MAX_DETECTIONS: a frame of the grid form
constexpr int kLifecycleThreads = 256;              // threads of every lifecycle workgroup: four wavefronts of 64
constexpr int kLifecycleWaves = kLifecycleThreads / 64;

// detection flags (lifecycle_det_flag)
constexpr unsigned char kLifecycleDetMatched = 0;     // slot_of_det >= 0: belongs to a target
constexpr unsigned char kLifecycleDetCandidate = 1;   // unmatched, all seven words finite: born unless the cap says no
constexpr unsigned char kLifecycleDetNonFinite = 2;   // unmatched, a NaN or inf word: never born

// the policy of a call (target_lifecycle_c)
struct LifecyclePolicy {
  int max_misses = 0;       // K >= 1: retire on the K-th consecutive frame without a match; 0: nobody
  int birth_type = -1;      // motion model 0..3 of new targets, -1: no births
  unsigned first_id = 0;    // born target j (ascending detection index) gets first_id + j
  long max_births = 0;      // cap per call: the lowest detection indices win
  double dt0 = 0.0, t_birth = 0.0;
  const double* Q = nullptr;   // as init_batch_typed with per_target_P0 = 0; all three null: the manager's own model parameters
  const double* R = nullptr;
  const double* P0 = nullptr;
  bool births() const { return birth_type >= 0; }
  bool defaults() const { return !Q && !R && !P0; }
};

// THE COUNTERS of one slot behind one call: has != 0 resets the run of misses and counts a hit, 0 lengthens the run; both
// saturate at 255.
TE_LC_HD inline unsigned char lifecycle_next_miss(unsigned char has, unsigned char miss) {
  return has ? (unsigned char)0 : (miss < 255 ? (unsigned char)(miss + 1) : (unsigned char)255);
}
TE_LC_HD inline unsigned char lifecycle_next_hits(unsigned char has, unsigned char hits) {
  return (has && hits < 255) ? (unsigned char)(hits + 1) : hits;
}
inline void lifecycle_count(unsigned char has, unsigned char& miss, unsigned char& hits) {
  miss = lifecycle_next_miss(has, miss);
  hits = lifecycle_next_hits(has, hits);
}
// STALE: K >= 1 and the new run of misses has reached K
TE_LC_HD inline bool lifecycle_stale(int max_misses, unsigned char miss) { return max_misses >= 1 && (int)miss >= max_misses; }
// a detection row with seven finite words (x - x == 0 fails for NaN and for +-inf)
TE_LC_HD inline bool lifecycle_row_finite(const double* r) {
  bool ok = true;
  for (int c = 0; c < 7; ++c) ok = ok && (r[c] - r[c] == 0.0);
  return ok;
}
TE_LC_HD inline unsigned char lifecycle_det_flag(int slot_of_det, const double* row) {
  if (slot_of_det >= 0) return kLifecycleDetMatched;
  return lifecycle_row_finite(row) ? kLifecycleDetCandidate : kLifecycleDetNonFinite;
}

// THE ORDERED COMPACTION's arithmetic: a workgroup owns kLifecycleThreads consecutive entries, a wavefront 64 of them.  An entry's
// position in the output = the flagged entries of the blocks before its own + of the wavefronts before its own in the block + of
// the lanes below its own in the wavefront (popcount of the ballot below the lane).
inline long lifecycle_blocks(long n) { return n <= 0 ? 1 : (n + kLifecycleThreads - 1) / kLifecycleThreads; }
TE_LC_HD inline int lifecycle_rank_in_wave(unsigned long long ballot, int lane) {
  const unsigned long long below = lane == 0 ? 0ull : (ballot & (~0ull >> (64 - lane)));
  int c = 0;
  for (unsigned long long b = below; b; b &= b - 1) ++c;
  return c;
}
// the born among `candidates` under the cap
inline long lifecycle_born(long candidates, long max_births) { return candidates < max_births ? candidates : max_births; }

// THE REFUSALS that need no handle, in the order the header lists them.  has_* say whether the pointer is there; the per-batch
// masks are the shard's to check (they depend on the batches' sizes).
inline void check_lifecycle_args(const LifecyclePolicy* p, bool have_info, long M, bool have_det, bool have_slot_of_det, long n_batches,
                                 bool have_masks, long retired_cap, bool have_retired) {
  const std::string pre = "target_estimation_amd: lifecycle: ";
  if (!p) throw std::invalid_argument(pre + "the policy is required");
  if (!have_info) throw std::invalid_argument(pre + "info is required");
  if (M < 0 || M > kLifecycleMaxDetections)
    throw std::invalid_argument(pre + "M must be 0.." + std::to_string(kLifecycleMaxDetections) + ", got " + std::to_string(M));
  if (p->max_misses < 0 || p->max_misses > 255) throw std::invalid_argument(pre + "max_misses must be 0..255, got " + std::to_string(p->max_misses));
  if (p->birth_type < -1 || p->birth_type > 3) throw std::invalid_argument(pre + "birth_type must be -1..3, got " + std::to_string(p->birth_type));
  if (p->max_births < 0) throw std::invalid_argument(pre + "max_births must be >= 0, got " + std::to_string(p->max_births));
  if (p->t_birth != p->t_birth || p->dt0 != p->dt0) throw std::invalid_argument(pre + "t_birth and dt0 must not be NaN");
  if (!p->defaults() && !(p->Q && p->R && p->P0)) throw std::invalid_argument(pre + "Q, R and P0 are given together or not at all");
  if (M > 0 && p->births() && (!have_det || !have_slot_of_det))
    throw std::invalid_argument(pre + "the detections and slot_of_det are required for births");
  if (n_batches < 0 || (n_batches > 0 && !have_masks)) throw std::invalid_argument(pre + "one mask per batch is needed");
  if (retired_cap < 0 || (retired_cap > 0 && !have_retired)) throw std::invalid_argument(pre + "retired_ids_out is required for retired_cap > 0");
}

// THE ID RANGE [first_id, first_id + born) must not wrap past 2^32 - 1
inline bool lifecycle_ids_wrap(unsigned first_id, long born) {
  return born > 0 && (unsigned long long)first_id + (unsigned long long)born - 1ull > 0xFFFFFFFFull;
}

}  // namespace te
