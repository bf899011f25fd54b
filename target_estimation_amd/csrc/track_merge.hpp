// track_merge.hpp -- host side of the duplicate-track kernels (track_merge.hip): "which two tracks follow the same object"
// (target_batch_c.h, target_manager_find_duplicates_dev / target_manager_retire_duplicates).  The rule -- the row,
// the classes, the pair, the survivor, the refusals -- is track_merge_plan.hpp; this header is the launches and the scratch.
//
// A CALL is this sequence on the shard's one stream; the number of launches depends on `rounds` and the number of batches alone,
// never on the data (every launch of a round after a settled one returns at once on the state's flag):
//   assoc_table_kernel<M, T, G, LAYOUT>   per batch, the association's own, with AssocTableArgs::sigma_in_w: rows (zhat, Sigma, tag)
//   merge_init_kernel                     nothing matched, counters and bucket counts zero
//   merge_classify_kernel                 per batch, a thread per row: reach2 from 2 Sigma_aa, the slot's hits and miss; eligible /
//                                         wide / none; an eligible row's bucket is counted, a wide row only counted
//   assoc_grid_scan_{blocks,sums,add}, assoc_grid_place_kernel   the grid form's, with zero detections (launch_assoc_grid_bin_rows)
//   per round:
//     merge_scan_kernel                   32 lanes per unmatched eligible row in bucket order: a lane per cell walks the ROW buckets
//                                         of the row's 27 cells; per visit the pair's C, its cofactor inverse, d2 and the box;
//                                         the lanes' picks are merged by the full key
//     merge_resolve_kernel                a thread per row, many workgroups: two rows that picked each other are a pair; each
//                                         writes its own words only; counts by integer atomics
//     merge_finish_kernel                 one thread: state = {pairs, rounds_run, settled}
//   merge_out_kernel                      per batch: dup, partner (batch, slot) from the partner's tag, d2
//   merge_info_kernel                     info = {pairs, rounds_run, settled, wide rows}
// Atomics: integer adds only (bucket counts, placement cursors, the wide count, the round's counts).  The order they leave inside
// a bucket reaches no output: every pick compares the full key (assoc_take_keyed).
#pragma once
#include <hip/hip_runtime.h>

#include "associate.hpp"
#include "dev_mem.hpp"
#include "track_merge_plan.hpp"

namespace te {

// The scratch of a shard's duplicate searches, owned by the Shard.  Grow-only.
class MergeScratch {
 public:
  MergeScratch() = default;
  MergeScratch(const MergeScratch&) = delete;
  MergeScratch& operator=(const MergeScratch&) = delete;
  void ensure(long rows, long buckets);
  // ... and for retire_duplicates: the search's outputs, the compaction, the block that crosses the bus
  void ensure_retire(long rows, long n_batches);

  DeviceBuf<AssocRow> table;           // [rows] MergeRows
  DeviceBuf<unsigned char> hits, miss; // [rows] the counters as the classify step read them
  DeviceBuf<int> bucket_of, order;     // [rows]
  DeviceBuf<int> partner, pick_idx;    // [rows] -1: none
  DeviceBuf<double> d2, pick_d2;       // [rows]
  DeviceBuf<int> count, start, cursor, sums;   // per bucket (start: + the total); the scan's block sums
  DeviceBuf<int> state, counters;      // {pairs, rounds_run, settled, 0}; {wide rows, pairs this round, open this round, 0}
  // retire: the mask and the partners per row; per batch the ascending list of duplicates and, gathered to the list's order, the
  // partners; the counts; info
  DeviceBuf<unsigned char> dup;
  DeviceBuf<int> partner_batch, partner_slot, list, list_batch, list_slot, csums, counts;
  PinnedBuf<int> host;                 // [n_batches counts][4 info][3 x rows: slots | partner batches | partner slots]

 private:
  long cap_rows_ = -1, cap_buckets_ = -1, cap_retire_rows_ = -1, cap_retire_batches_ = -1;
};

struct MergeBatchIn {
  long size = 0;
  const unsigned char* hits = nullptr;   // the batch's counters (device, read only)
  const unsigned char* miss = nullptr;
};
// what a batch's slots get: dup is required, the others may be null
struct MergeSlotOut {
  unsigned char* dup = nullptr;
  int* partner_batch = nullptr;
  int* partner_slot = nullptr;
  double* d2 = nullptr;
};

// init + classify + binning + `rounds` rounds over s.table (`rows` MergeRows, the batches' concatenated)
void launch_merge_match(const MergeScratch& s, long rows, const MergeBatchIn* in, int n_batches, double gate, double cell, int rounds,
                        int min_hits, long buckets, hipStream_t st);
void launch_merge_out(const MergeScratch& s, long row_offset, long size, const MergeSlotOut& out, hipStream_t st);
void launch_merge_info(const MergeScratch& s, int* info, hipStream_t st);
// list_batch[k], list_slot[k] = the partner of slot list[k], k < *count (device), for a batch of `size` slots at row_offset
void launch_merge_gather(const MergeScratch& s, long row_offset, long size, const int* count_dev, hipStream_t st);

}  // namespace te
