// associate_grid.hpp -- host side of the GRID form of the association (associate_grid.hip; target_batch_c.h,
// target_batch_associate_grid*).  The rule -- the box, the cell map, narrow and wide slots, the hash, the keyed
// pick -- is associate_grid_plan.hpp; this header is the launches.  The scratch is AssocScratch's (associate.hpp).
//
// A CALL is this sequence on one stream; the number of launches depends on `rounds` alone, never on the data (every launch of a
// round after a settled one returns at once on the state's flag):
//   assoc_table_kernel<M, T, G, LAYOUT>   per batch, as in the brute-force form, with AssocTableArgs::sdiag set: S's diagonal too
//   assoc_grid_init_kernel                nothing matched, counters and bucket counts zero
//   assoc_grid_classify_kernel            a thread per row: reach2, narrow / wide / none; a narrow row's bucket is counted, a wide
//                                         row appended to the wide list
//   assoc_grid_bin_dets_kernel            a thread per detection: its bucket (none for a non-finite position), counted
//   assoc_grid_scan_{blocks,sums,add}     exclusive scan of the counts: every bucket's start in the index list
//   assoc_grid_place_kernel               detections and narrow rows into the bucket-grouped index list
//   per round:
//     assoc_grid_scan_rows_kernel         32 lanes per narrow row, rows in bucket order: a lane per cell walks the detection buckets
//                                         of the row's 27 cells; the lanes' picks are merged by the full key
//     assoc_grid_scan_wide_kernel         a fixed grid striding over the wide list: every wide row against all detections through LDS
//     assoc_grid_scan_dets_kernel         32 lanes per detection: the row buckets of its 27 cells, then the wide list through LDS
//     assoc_grid_resolve_kernel           a thread per detection, many workgroups: the mutual pairs; counts by integer atomics
//     assoc_grid_finish_kernel            one thread: state[0..2] exactly as the brute-force resolve sets them
//   assoc_scatter_kernel<T>, assoc_dets_kernel   the brute-force form's, then assoc_grid_info_kernel: info[3] = the wide slots
// Atomics: integer adds only (bucket counts, placement cursors, the wide list's length, the round's counts).  The order they leave
// inside a bucket and inside the wide list reaches no output: every pick compares the full key (assoc_take_keyed).
#pragma once
#include <hip/hip_runtime.h>

#include "associate.hpp"
#include "associate_grid_plan.hpp"

namespace te {

// the bucket counts of a call (detection buckets, row buckets) from the counts that could be binned at most
struct AssocGridBuckets {
  long dets = 0, rows = 0;
  long total() const { return dets + rows; }
};
inline AssocGridBuckets plan_assoc_grid_call(long rows, long M, long forced_buckets) {
  AssocGridBuckets b;
  b.dets = plan_assoc_grid_buckets(M, forced_buckets);
  b.rows = plan_assoc_grid_buckets(rows, forced_buckets);
  return b;
}

// init + binning + `rounds` rounds over a table of `rows` rows (with s.grid_sdiag filled) and det [M][7] (device)
void launch_assoc_grid_match(const AssocScratch& s, long rows, const double* det, long M, double gate, double cell, int rounds,
                             const AssocGridBuckets& buckets, hipStream_t st);
// after launch_assoc_dets: info[3] = the number of wide slots
void launch_assoc_grid_info(const AssocScratch& s, int* info, hipStream_t st);
// The scan and place kernels above with ZERO detections, for a caller that bins rows alone (track_merge.hpp): count [buckets] the
// entries per bucket, bucket_of [rows] (-1: binned nowhere); start [buckets + 1], cursor [buckets] and order [rows] are written,
// sums is room for assoc_grid_scan_blocks(buckets) + 1 ints.  buckets a power of two.
long assoc_grid_scan_blocks(long buckets);
void launch_assoc_grid_bin_rows(const int* bucket_of, int* count, int* start, int* cursor, int* sums, int* order, long rows, long buckets,
                                hipStream_t st);

}  // namespace te
