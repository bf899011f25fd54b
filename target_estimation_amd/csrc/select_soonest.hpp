// select_soonest.hpp -- host side of the selection kernels (select_soonest.hip): "which k targets cross the sphere soonest" over
// the query outputs a tick leaves in device memory (delta [n], pose [n][7]; target_batch_c.h, target_batch_select_soonest*).
//
// ALGORITHM: a local top-k per workgroup, merged by a tree of fixed depth -- always three launches, whatever n and k:
//   1  soonest_scan_kernel   G workgroups of kSoonestChunk threads.  A workgroup walks its chunks of the parts' delta (and ok)
//                            arrays, keeps the candidates whose key is below the k-th best it has seen, and writes its k best keys.
//   2  soonest_merge_kernel  ceil(G / kSoonestFanIn) workgroups, each merging kSoonestFanIn of those lists into one.
//   3  soonest_merge_kernel  one workgroup merges the middle lists, orders the k rows and gathers slot, batch, delta and pose.
// A workgroup's list lives in LDS as 512 keys.  Until its first sort all 512 places collect; from then on the lower half holds the
// 256 best so far, sorted, and the upper half collects.  When a round's survivors do not fit, one bitonic sort of the 512 folds
// them in and renews the threshold; a list that collected nothing since its last sort, or a single input list, is not sorted again.
// A call of at most 64 chunks keeps to 32 first-stage workgroups, so one middle workgroup merges them all and the last stage
// passes one list on.  Survivors are placed by a ballot prefix sum; whatever order that gives is removed by the sort on the full
// (delta, batch, slot) key, so the result is a function of the inputs alone.  No
// atomics, no flags, no workgroup waits for another; every loop's trip count is known when it starts.
// Why not a radix select: its passes over the key's 8 + 8 bytes are launches or grid-wide waits; this reads delta once, and a
// result of <= 256 rows fits the list a workgroup can sort in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_mem.hpp"
#include "select_soonest_plan.hpp"

namespace te {

// one batch's arrays in a launch: n entries, candidates per soonest_candidate; batch = the index its rows carry
struct SoonestPart {
  const double* delta;
  const unsigned char* ok;   // or null: every entry passes
  const double* pose;        // [n][7], or null in every part: no gather
  long n;
  int batch;
};

// where a launch writes (device memory): rows count .. k-1 get the filler.  batch and pose may be null.
struct SoonestOut {
  int* batch;
  int* slot;
  double* delta;
  double* pose;   // [k][7]
  int* count;
};

// The scratch of a shard's selections, owned by the Shard: the workgroups' lists of one call, a device result for the host forms
// and its pinned mirror.  All calls of a shard are enqueued on the shard's one stream, so consecutive calls may share it.  Sized
// once, at the first call (the knob bounds the grid), so a warm call allocates nothing; released through device_free.
class SoonestScratch {
 public:
  SoonestScratch() = default;
  SoonestScratch(const SoonestScratch&) = delete;
  SoonestScratch& operator=(const SoonestScratch&) = delete;
  void ensure(int max_wgs);            // allocates on first use, for first stages of up to max_wgs workgroups (ShardSettings::soonest_max_wgs)
  int max_wgs() const { return max_wgs_; }
  SoonestKey* lists() const { return lists_.get(); }
  // the device result of the host forms and its pinned mirror: batch int[K] | slot int[K] | delta double[K] | pose double[K][7] | count int
  char* result_dev() const { return result_dev_.get(); }
  char* result_host() const { return result_host_.host(); }
  static constexpr size_t kOffBatch = 0, kOffSlot = kSoonestMaxK * 4, kOffDelta = kSoonestMaxK * 8, kOffPose = kSoonestMaxK * 16,
                          kOffCount = kSoonestMaxK * 72, kResultBytes = kSoonestMaxK * 72 + 8;
  SoonestOut result_out(bool with_pose) const;

 private:
  int max_wgs_ = 0;
  DeviceBuf<SoonestKey> lists_;
  DeviceBuf<char> result_dev_;
  PinnedBuf<char> result_host_;
};

// Enqueue the three launches on `st`.  parts [n_parts <= kSoonestMaxParts] (host array; n_parts may be 0: an empty result).
// Arguments are the caller's to check (check_soonest_args); scratch.ensure() has been called.
void launch_select_soonest(const SoonestPart* parts, int n_parts, double delta_lo, double delta_hi, int k, const SoonestOut& out,
                           const SoonestScratch& scratch, hipStream_t st);
// the launches + the copy of the device result to the pinned mirror + a synchronisation; rows [k] filled, returns count
// (in two halves, so that a manager enqueues on every shard before it waits for any: begin = launches + copy, end = wait + rows)
void select_soonest_begin(const SoonestPart* parts, int n_parts, double delta_lo, double delta_hi, int k, bool with_pose,
                          SoonestScratch& scratch, hipStream_t st);
long select_soonest_end(int k, bool with_pose, SoonestScratch& scratch, hipStream_t st, SoonestRow* rows);
long select_soonest_to_host(const SoonestPart* parts, int n_parts, double delta_lo, double delta_hi, int k, bool with_pose,
                            SoonestScratch& scratch, hipStream_t st, SoonestRow* rows);

}  // namespace te
