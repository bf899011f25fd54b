// lifecycle.hpp -- host side of the track-lifecycle kernels (lifecycle.hip): "which targets of an unlabelled frame are gone, which
// detections are new" (target_batch_c.h, target_manager_lifecycle).  The rule -- counters, stale, born, the block
// arithmetic, the refusals -- is lifecycle_plan.hpp; this header is the launches and the scratch.
//
// A CALL is this sequence on the shard's one stream (Shard::lifecycle):
//   per non-empty batch:
//     lifecycle_count_kernel        a thread per slot: the slot's new (miss, hits) from its mask byte INTO THE SCRATCH, and the
//                                   stale flag
//     lifecycle_scan_blocks_kernel  the ORDERED compaction, stage 1: per workgroup the number of flagged entries (ballot +
//                                   popcount per wavefront, LDS across the four wavefronts)
//     lifecycle_scan_sums_kernel    stage 2, one workgroup: the exclusive scan of the block counts (with a carry, whatever their
//                                   number) and the total
//     lifecycle_scatter_kernel      stage 3: every flagged entry's index to its rank -- the stale slots in ascending order
//   with births:
//     lifecycle_det_flag_kernel     a thread per detection: matched / unmatched and finite / unmatched and not
//     the three compaction stages over the candidates (their list ascending: the first min(count, max_births) are born), and the
//     first two over the non-finite ones (their count alone)
//   one copy of the counts into the pinned block, a wait; one copy per batch with stale slots of its list into the same block,
//   a wait.  The host checks (retired_cap, the id range) -- nothing but scratch has been written so far.
//   per non-empty batch:
//     lifecycle_commit_kernel       the new counters from the scratch into the batch's own
//   then Batch::erase_slots per batch with stale slots (its launches, plus lifecycle_moves_kernel for the counters of the survivors
//   that fill the holes) and one Batch::append_gathered (lifecycle_gather_kernel: det[j] -> the init staging [born][7], a thread per
//   (row, word); then the batch's own init launcher).
// No atomics: every word has one writer per launch; plain vector stores only; the order of every list is the index order.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_mem.hpp"
#include "lifecycle_plan.hpp"

namespace te {

// The scratch of a shard's lifecycle calls, owned by the Shard.  Grow-only: a call allocates only when it is larger than every
// call before it on this shard.  Entries: the slots of every batch, batch after batch, then the detections.
class LifecycleScratch {
 public:
  LifecycleScratch() = default;
  LifecycleScratch(const LifecycleScratch&) = delete;
  LifecycleScratch& operator=(const LifecycleScratch&) = delete;
  void ensure(long rows, long dets, long n_batches);

  DeviceBuf<unsigned char> new_miss, new_hits;   // [rows]
  DeviceBuf<unsigned char> flag;                 // [rows + dets]
  DeviceBuf<int> list;                           // [rows + dets]: per batch its stale slots, then the candidate detections
  DeviceBuf<int> sums;                           // [blocks(rows + dets) + n_batches + 1]: the block counts / offsets of one compaction at a time
  DeviceBuf<int> counts;                         // [n_batches + 2]: stale per batch | candidates | non-finite unmatched
  PinnedBuf<int> host;                           // the ONE block that crosses the bus: [counts (n_batches + 2)] [stale lists]
  long host_lists_cap() const { return cap_rows_; }

 private:
  long cap_rows_ = -1, cap_entries_ = -1, cap_batches_ = -1;
};

// new counters of n slots into the scratch, stale flags (K = max_misses)
void launch_lifecycle_count(const unsigned char* has, const unsigned char* miss, const unsigned char* hits, unsigned char* new_miss,
                            unsigned char* new_hits, unsigned char* flag, long n, int max_misses, hipStream_t st);
// flags of M detections (lifecycle_det_flag)
void launch_lifecycle_det_flags(const double* det, const int* slot_of_det, unsigned char* flag, long M, hipStream_t st);
// the ordered compaction of the entries i < n with flag[i] == want: list (or null: count only) receives them ascending, *count_out
// their number.  sums: room for lifecycle_blocks(n) ints.
void launch_lifecycle_compact(const unsigned char* flag, unsigned char want, long n, int* sums, int* list, int* count_out, hipStream_t st);
void launch_lifecycle_commit(unsigned char* miss, unsigned char* hits, const unsigned char* new_miss, const unsigned char* new_hits, long n,
                             hipStream_t st);
// the counters of the survivors that fill the holes of a batched erase (every source lies above every destination)
void launch_lifecycle_moves(unsigned char* miss, unsigned char* hits, const int* src, const int* dst, long m, hipStream_t st);
// det[rows[r]] -> out[r], r < count, seven words each
void launch_lifecycle_gather(const double* det, const int* rows, long count, double* out, hipStream_t st);

}  // namespace te
