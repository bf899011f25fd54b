// associate.hpp -- host side of the association kernels (associate.hip): "which detection of an unlabelled frame belongs to which
// target" (target_batch_c.h, target_batch_associate*).  The rule -- the table row, S^-1, d^2, the candidate and tie
// rules, the grid -- is associate_plan.hpp; this header is the launches and the scratch.
//
// A CALL is this sequence on one stream, whatever the number of rounds (every launch of a round after a settled one returns at once
// on the state's flag):
//   assoc_table_kernel<M, T, G, LAYOUT>   per batch, a thread per slot: the slot's table row (zhat, W = S^-1, tag) in double.  The
//                                         batches' rows are concatenated in target_manager_get_batch order: row = offset + slot.
//   assoc_init_kernel                     nothing matched, counters zero
//   per round:
//     assoc_scan_rows_kernel              target-major: a thread owns a table row in registers and walks its chunk of the detections,
//                                         staged through LDS in tiles; writes the row's partial minimum (d^2, detection) of the chunk
//     assoc_scan_dets_kernel              detection-major, the mirror image: table rows staged through LDS at 80 B per row
//     assoc_resolve_kernel                merges the partials in ascending chunk order, matches the mutual pairs, counts, and sets the
//                                         settled flag
//   assoc_scatter_kernel<T>               per batch: SoA measurements, mask and filler rows in the form target_batch_step reads
//   assoc_dets_kernel                     the per-detection arrays and info
// No atomics: every word has one writer per launch; plain vector stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "associate_plan.hpp"
#include "dev_mem.hpp"

namespace te {

struct AssocTableArgs {
  char* rec;                 // the records as stored (read, never written)
  const void* qr;            // the batch's [Q | R] row in its precision, or (cls != null) its table of rows
  const int* cls;            // per-slot parameter class, or null
  const double* tile_blk;    // the batch's uniform tiles, honoured read-only (null: none)
  const int* tile_uni;
  long size;                 // slots of the batch
  double dt;
  AssocRow* rows;            // [size]: the batch's part of the call's table
  int batch_index;           // what the rows' tags carry
  double* sdiag = nullptr;   // [size][3]: the diagonal of the S that was inverted, for the grid form (associate_grid.hpp); null: not written
  bool sigma_in_w = false;   // the row's six W words receive Sigma (before R is added) instead of W: a MergeRow (track_merge_plan.hpp)
};
// the launcher of a (model, precision, lanes per target, layout as LayoutInfo reports it, shared-axes form), or null
using AssocTableLaunch = void (*)(const AssocTableArgs&, hipStream_t);
AssocTableLaunch assoc_table_launcher(int type, int dtype, int g, int layout, bool shared_axes);

// The scratch of a shard's associations, owned by the Shard (all its calls are enqueued on the shard's one stream, so consecutive
// calls may share it).  Grow-only: a call allocates only when it is larger than every call before it on this shard.
class AssocScratch {
 public:
  AssocScratch() = default;
  AssocScratch(const AssocScratch&) = delete;
  AssocScratch& operator=(const AssocScratch&) = delete;
  // room for `rows` table rows, `dets` detections and the two scans' partials (entries x chunks)
  void ensure(long rows, long dets, long part_rows, long part_dets);
  // ... and for the host forms: the staged detections, the device result and its pinned mirror
  void ensure_host(long dets);
  // ... and for the grid form (associate_grid.hpp): `buckets` = detection buckets + row buckets
  void ensure_grid(long rows, long dets, long buckets);

  DeviceBuf<AssocRow> table;
  DeviceBuf<int> det_of_row;       // [rows]  -1: unmatched
  DeviceBuf<double> d2_of_row;     // [rows]  the target-major scan's d^2 of the match, -1: none
  DeviceBuf<int> row_of_det;       // [dets]
  DeviceBuf<double> d2_of_det;     // [dets]  the detection-major scan's
  DeviceBuf<double> part_rows_d2;  // [chunks][rows]
  DeviceBuf<int> part_rows_idx;
  DeviceBuf<double> part_dets_d2;  // [chunks][dets]
  DeviceBuf<int> part_dets_idx;
  DeviceBuf<int> state;            // {matched, rounds_run, settled, 0}
  // grid form: S's diagonal and the box [rows][3]; the bucket of every detection, then of every row (-1: binned nowhere);
  // per bucket (detection buckets first, then row buckets) the count, the exclusive start (+ the total) and the placement cursor;
  // the scan's block sums; the bucket-grouped index list (detections, then narrow rows); the wide rows; {wide, matched, open, 0}
  DeviceBuf<double> grid_sdiag, grid_reach2;
  DeviceBuf<int> grid_bucket_of, grid_count, grid_start, grid_cursor, grid_sums, grid_order, grid_wide, grid_counters;
  // host forms: det [dets][7] | the result: slot int[dets] | batch int[dets] | d2 double[dets] | info int[4]
  DeviceBuf<double> det_stage;
  DeviceBuf<char> result_dev;
  PinnedBuf<char> result_host;
  static size_t off_slot(long) { return 0; }
  static size_t off_batch(long dets) { return (size_t)dets * 4; }
  static size_t off_d2(long dets) { return (size_t)dets * 8; }
  static size_t off_info(long dets) { return (size_t)dets * 16; }
  static size_t result_bytes(long dets) { return (size_t)dets * 16 + 16; }

 private:
  long cap_rows_ = 0, cap_dets_ = 0, cap_part_rows_ = 0, cap_part_dets_ = 0, cap_host_ = 0;
  long cap_grid_rows_ = 0, cap_grid_dets_ = 0, cap_grid_buckets_ = 0;
};

// init + `rounds` rounds over a table of `rows` rows and det [M][7] (device); forced_chunks: TE_ASSOC_COL_CHUNKS or 0
void launch_assoc_match(const AssocScratch& s, long rows, const double* det, long M, double gate, int rounds, int forced_chunks, hipStream_t st);
// what a batch's slots get: any pointer may be null
struct AssocSlotOut {
  void* meas = nullptr;               // SoA [7][ld] in the batch precision
  long ld = 0;
  unsigned char* has_meas = nullptr;  // [size]
  int* det_of_slot = nullptr;         // [size]
  double* d2_of_slot = nullptr;       // [size]
};
void launch_assoc_scatter(int dtype, const AssocScratch& s, long row_offset, long size, const double* det, const AssocSlotOut& out, hipStream_t st);
// the per-detection arrays (any may be null) and info [4]
void launch_assoc_dets(const AssocScratch& s, long M, int* slot_of_det, int* batch_of_det, double* d2_of_det, int* info, hipStream_t st);

}  // namespace te
