// shard.hpp -- everything a TargetManager holds on ONE device: the batches, the id -> (batch, slot) table, the device-side id
// resolution, the recorded all-batches sequences and the row maps of getEstAllById.  A manager owns one Shard per device it
// spans (target_manager.hpp), exactly one unless setDevices said otherwise.
//
// CONTRACT, for every method: the caller holds the owning manager's lock and has made the shard's device the current HIP
// device.  A Shard has no lock of its own, writes no log file, reads no environment and knows no other shard; what it needs of
// the manager's settings it reads through `ShardSettings`, which the manager owns and may change between calls.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch_store.hpp"
#include "id_table.hpp"
#include "row_split.hpp"
#include "step_variant.hpp"
#include "track_merge.hpp"

namespace te {

struct ResolveCounters;   // id_resolve.hpp (kernels: included by shard.cpp only)

// true if Q, R and the n_P0 covariances have no entry between different axis groups (te_layout.hpp)
bool is_axis_separable(int type, const double* Q, const double* R, const double* P0, long n_P0);
// true if, on top of that, the axes of every kind (x, y, z; roll, pitch, yaw of angular_rates) have equal Q blocks, R entries and
// blocks in each of the n_P0 covariances, compared exactly: what the shared-axes storage form needs (te_layout.hpp, Batch)
bool axes_shareable(int type, const double* Q, const double* R, const double* P0, long n_P0);
// unit quaternion [x y z w] -> rotation matrix (row-major), Eigen's Quaterniond::toRotationMatrix
void host_quat_to_rot(const double* q, double* R);

// row i of a sphere query's outputs (any may be null) for a target that does not exist or never meets the sphere
inline void no_intersection(long i, double* delta, double* pose, unsigned char* converged, double* filt) {
  if (delta) delta[i] = -1;
  if (converged) converged[i] = 0;
  if (pose) { for (int c = 0; c < 6; ++c) pose[i * 7 + c] = 0.0; pose[i * 7 + 6] = 1.0; }
  if (filt) { filt[i * 2] = 0.0; filt[i * 2 + 1] = 0.0; }
}

// the manager's settings as its shards read them (one copy, in the manager)
struct ShardSettings {
  int dtype = F64;
  int lanes = 0;              // lanes code asked for at construction, 0 = automatic (Shard::chooseLayout)
  bool verbose = false;       // TARGET_ESTIMATION_VERBOSE
  bool keep_meas = false;     // setKeepMeasurement: batches created later inherit the measured-pose rows
  int filters_length = 250;   // setIntersectionFiltersLength
  long small_batch_most = 0;  // the largest host-array call that goes through the one-target queue (TE_SMALL_BATCH_QUEUE)
  bool population_tick = true;   // TE_POPULATION_TICK
  bool uniform_tiles = true;     // TE_UNIFORM_TILES / TargetManager::setUniformTiles: new shared-axes batches keep uniform tiles (Batch)
  bool shared_axes = true;       // TE_SHARED_AXES / TargetManager::setSharedAxes: new fp64 batches may use the shared-axes storage form (Batch)
  UpdateGate gate[4];            // TargetManager::setUpdateGate: the by-id update policy per model type; batches created later inherit it
  int soonest_max_wgs = kSoonestDefaultMaxWgs;   // TE_SELECT_SOONEST_MAX_WGS: the cap on the selection's first-stage workgroups (select_soonest.hpp)
  int assoc_col_chunks = 0;      // TE_ASSOC_COL_CHUNKS: the column chunks of the association scans, 0 = planned (associate_plan.hpp)
  long assoc_grid_buckets = 0;    // TE_ASSOC_GRID_BUCKETS: the buckets of the grid form's hash, 0 = planned (associate_grid_plan.hpp)
};

// one batch of a manager-level selection (TargetManager::selectSoonest): the query outputs of target_batch_sequence_c and the
// batch's mask.  delta == null: the batch is skipped.
struct SoonestSpec {
  const double* delta = nullptr;
  const double* pose = nullptr;
  const unsigned char* ok = nullptr;
};

// one target's log rows, formatted per channel (TargetManager::log); batch: the shard's batch index as logCollect leaves it
struct LogRow { unsigned id = 0; int batch = 0; std::string ch[7]; };

class Shard {
 public:
  // `owner_lock`: the manager's mutex, handed to every Batch (Batch::owner_lock); the shard itself never takes it
  Shard(const ShardSettings& settings, std::mutex* owner_lock);
  ~Shard();
  Shard(const Shard&) = delete;
  Shard& operator=(const Shard&) = delete;

  // ---- what the manager reads
  size_t size() const { return targets_.size(); }
  bool contains(unsigned id) const { return targets_.contains(id); }
  std::vector<unsigned> sortedIds() const { return targets_.sorted_ids(); }   // ascending, as the reference's std::map iteration
  const std::vector<std::unique_ptr<Batch>>& batches() const { return batches_; }
  const Batch* batchOf(unsigned id) const;   // null: unknown id
  Batch* batchOfType(int type);
  hipStream_t stream() const { return stream_; }
  void setStream(hipStream_t s);
  void keepMeasurementChanged();   // settings.keep_meas to every batch; drops the recorded sequences
  void synchronize();

  // ---- by id (return values and messages of the manager's methods of the same purpose)
  bool init(int type, unsigned id, double t0, const double* Q, const double* R, const double* P0, const double* p0, const double* v0,
            const double* a0);   // false: the id exists already (said so)
  // (update and outputsOne are the reference's one-target cycle, a latency path measured in nanoseconds per call: inline)
  bool update(unsigned id, double dt, const double* meas) {   // meas null: prediction only
    Loc loc;
    if (!find(id, loc)) { notFound(id); return false; }
    Batch& b = *batches_[(size_t)loc.batch];
    if (meas && b.update_gate().on()) {   // (off: one load and one compare on the latency path)
      if (const char* why = b.update_gate_refusal()) throw std::runtime_error(why);
    }
    b.step_one(loc.slot, dt, meas);
    return true;
  }
  bool erase(unsigned id);
  bool outputsOne(unsigned id, double* pose7, double* twist6, double* acc6, bool at_time, double t1) {
    Loc loc;
    if (!find(id, loc)) return false;
    batches_[(size_t)loc.batch]->outputs_one(loc.slot, pose7, twist6, acc6, at_time, t1);
    return true;
  }
  bool measuredPose(unsigned id, double* pose7);
  bool dims(unsigned id, int& n, int& m);
  bool modelMatrices(unsigned id, double* Q, double* R, double* P0);
  bool time(unsigned id, double& t);
  int state(unsigned id, double* x, double* P);
  long long numberMeasurements(unsigned id);
  int rejectionRun(unsigned id);   // the target's run of consecutive gate rejections (Batch::rejection_run), -1: unknown id
  bool trackCounts(unsigned id, int& miss, int& hits);   // the target's track counters (Batch::track_count); false: unknown id
  double intersectTime(unsigned id, double t1, const double* origin, double radius);
  bool intersectPose(unsigned id, double t1, const double* origin, double radius, double* pose7, double* delta);

  // ---- host arrays
  long initBatch(int type, const unsigned* ids, long n, double t0, const double* Q, const double* R, const double* P0, bool per_target_P0,
                 const double* p0, const double* v0, const double* a0);
  long initBatchClasses(int type, const unsigned* ids, long n, double t0, long n_classes, const double* Q, const double* R, const double* P0,
                        const unsigned* class_of, const double* p0, const double* v0, const double* a0);
  void updateAll(double dt);
  // nis_out / event_out [n] (or null): what the update policy reports per entry (Batch: "the update policy of the by-id paths");
  // -2 / 0 for an unknown id.  With them the call flushes the one-target queue before it returns.
  long updateBatch(const unsigned* ids, long n, double dt, const double* meas, const unsigned char* has_meas, double* nis_out = nullptr,
                   unsigned char* event_out = nullptr);
  // The policy of settings.gate[type] to every batch of the model (flushes their queues).
  void updateGateChanged(int type);
  // throws, before anything is stepped, if a by-id update with measurements of these ids touches a batch that has a policy and
  // cannot serve it (Batch::update_gate_refusal)
  void checkUpdateGate(const unsigned* ids, long n) const;
  // 1 / 0: would by-id updates of the model's batch be served under settings.gate[type]; -1: no such batch
  int updateGateServed(int type) const;
  long eraseBatch(const unsigned* ids, long n, std::vector<unsigned>& erased);   // appends the ids that went away
  long getPoseBatch(const unsigned* ids, long n, double* pose, double* twist, double* acc, unsigned char* found, bool at_time, double t1);
  long getStateBatch(const unsigned* ids, long n, double* x, double* P);
  long intersectGatedBatch(const unsigned* ids, long n, double t1, double pos_th, double ang_th, const double* origin, double radius,
                           double* delta, double* pose, unsigned char* converged, unsigned char* found, double* filt);
  long intersectBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, double* delta, double* pose,
                      unsigned char* found);

  // ---- every batch at once (TargetManager::stepSequenceAll, live*All, posesToDevice, getEstAllById, log)
  bool populationTick() const;   // the tick of all batches as one launch (kf_population.hpp)
  // sched: the call's time-step schedule (dt_schedule.hpp; by default none): tick s of every batch runs with sched.dt[s]
  void stepSequenceAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, bool query, const double* origin, double radius,
                       int use_graph, const DtSchedule& sched = DtSchedule{});
  long seqRecordings() const { return seq_graphs_.recordings(); }   // all-batches recordings made so far
  // A temporally fused replay of every batch (target_manager_step_fused_all): for every batch, bit for bit, what
  // Batch::step_fused_gated(n_ticks, dt, spec..., sched) leaves.  ONE launch of kf_step_population_fused_kernel where plan_fused_all
  // (step_variant.hpp) says so: the population rule holds once every batch is expanded from the shared-axes form, no batch has a
  // pose stream in the call or keeps measured-pose rows, a schedule fits one table, and either no batch carries a stream, gate or
  // policy (the plain loop) or every non-empty batch carries at least its NIS rows (the gated loop).  Everything else is served
  // inside the call by the per-batch calls in batch order.  Every refusal of every batch's call is made before anything is
  // enqueued or changed (the storage form included); specs[b].ring_ticks must be 0, delta_dev and pose_dev are not read.
  void stepFusedAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, const DtSchedule& sched = DtSchedule{});
  // 1: such a call -- gated: every batch with NIS rows; scheduled: with a time-step schedule -- would be one launch now; 0: per batch
  int fusedAllServed(bool gated, bool scheduled) const;
  // THE k SOONEST CROSSINGS of all this shard's batches together (select_soonest.hpp): specs [batches().size()], batch i's rows
  // carry the index first_batch + i.  One set of three launches on the shard's stream, the first stage's grid split over the
  // batches by cumulative workgroup counts.  It reads no record of any batch (Batch::select_soonest_dev says what follows).
  //   checkSelectSoonest   what is refused about the specs (more batches than a launch takes, a pose gather from a batch without
  //                        pose rows); throws, nothing enqueued.  The window and k are the manager's to check.
  //   selectSoonestDev     into device memory, no host wait
  //   selectSoonestBegin   into the scratch's device result and, by one copy, its pinned mirror; no host wait
  //   selectSoonestEnd     waits for that copy: rows [k] on the host; returns count
  void checkSelectSoonest(const SoonestSpec* specs, long n_specs, bool with_pose) const;
  void selectSoonestDev(const SoonestSpec* specs, long n_specs, int first_batch, double lo, double hi, int k, const SoonestOut& out);
  void selectSoonestBegin(const SoonestSpec* specs, long n_specs, int first_batch, double lo, double hi, int k, bool with_pose);
  long selectSoonestEnd(int k, bool with_pose, SoonestRow* rows);
  // POSITION COVARIANCE AND TIME SPREAD AT THE CROSSINGS (crossing_cov.hpp; Batch::crossing_cov_dev says what is computed and
  // what is left alone).
  //   crossingCovDev    the rows a manager-level selection left on the device: batch_dev / slots_dev / delta_dev [n], batch entries
  //                     are the shard's batch indices.  One launch per batch of the shard, each serving the rows that carry its index,
  //                     and one that writes the filler into the rows that carry no batch of the shard: every row is written once.
  //                     No allocation, no host wait.  Everything is checked before anything is enqueued.
  //   crossingCovBatch  by id, host arrays: delta [n] is the caller's (e.g. of intersectBatch); unknown ids get the filler.
  //                     Runs the queued one-target steps first.  Returns the number of ids found.
  void crossingCovDev(double t1, const double* origin, double radius, const int* batch_dev, const int* slots_dev, const double* delta_dev,
                      long n, double sigma_r_max, double sigma_t_max, double* cov_dev, double* sigma_dev,
                      unsigned char* ok_dev);
  long crossingCovBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, const double* delta,
                        double sigma_r_max, double sigma_t_max, double* cov, double* sigma, unsigned char* ok);
  // ASSOCIATION OF UNLABELLED DETECTIONS with the targets of every batch of this shard together (associate.hpp; associate_batches
  // says what is launched, Batch::assoc_table_dev what is left alone): out [batches().size()], batch entries of batch_of_det are the
  // shard's batch indices.  associateDev: everything in device memory, no host wait.  associate: detections from host memory, the
  // per-detection rows back with ids; returns the matched count.
  // grid_cell > 0: the grid form (associate_grid.hpp), 0: the brute-force form.
  void associateDev(double dt, const double* det_dev, long M, double gate, long rounds, const AssocSlotOut* out, long n_out,
                    int* slot_of_det_dev, int* batch_of_det_dev, double* d2_of_det_dev, int* info_dev, double grid_cell = 0.0);
  long associate(double dt, const double* det, long M, double gate, long rounds, const AssocSlotOut* out, long n_out, unsigned* ids_of_det,
                 int* batch_of_det, int* slot_of_det, double* d2_of_det, long* unmatched, long* n_unmatched, int* info, double grid_cell = 0.0);
  // THE TRACK LIFECYCLE behind a tick that consumed an association (lifecycle.hpp lists the launches; lifecycle_plan.hpp is the rule):
  // has_dev [n_masks] the batches' masks in batch order, det_dev [M][7] / slot_of_det_dev [M] the frame and what the association
  // wrote, all device memory and only read.  The plan -- every slot's new counters, the stale slots of every batch ascending, the
  // born detections ascending -- is formed in the shard's scratch and read back (counts and stale slots only); every refusal that
  // depends on it (retired_cap, the id range) is made before anything but scratch is written.  Then the counters are committed,
  // the stale slots erased (Batch::erase_slots, the id table as eraseBatch keeps it) and the born rows appended
  // (Batch::append_gathered) to the batch initBatch(p.birth_type, ...) would use.  p.Q / R / P0 are resolved by the manager (never
  // null with births on).  retired_ids_out [retired_cap]: per batch in batch order, ascending former slot.  info [6]: see the C header.
  // Waits on the host; changes sizes: what erase and append do to recordings, tiles, storage forms and sessions, it does.
  void lifecycle(const double* det_dev, const int* slot_of_det_dev, long M, const unsigned char* const* has_dev, long n_masks,
                 const LifecyclePolicy& p, unsigned* retired_ids_out, long retired_cap, long* info);
  // DUPLICATE TRACKS (track_merge.hpp lists the launches; track_merge_plan.hpp is the rule): two tracks of this shard that follow the
  // same object.  findDuplicatesDev: out [n_out] per batch in batch order, everything in device memory, no host wait, no
  // allocation after the first call of at least that size; reads the records and counters as stored.  retireDuplicates: the same
  // search into the shard's scratch, each batch's mask compacted ascending (launch_lifecycle_compact), the counts, then the lists
  // with their partners read back; both sides translated to ids BEFORE anything moves; cap checked; only then Batch::erase_slots
  // per batch and the id table as eraseBatch keeps it.  info [4] = {retired, rounds_run, settled, wide}.  Waits on the host.
  void findDuplicatesDev(double dt, double gate, long rounds, double cell, int min_hits, const MergeSlotOut* out, long n_out, int* info_dev);
  void retireDuplicates(double dt, double gate, long rounds, double cell, int min_hits, unsigned* retired_ids_out, unsigned* kept_ids_out,
                        long cap, long* info);
  void liveStartAll(double dt, const Batch::SeqSpec* specs, long n_specs, long first_entry, long max_ticks, double idle_limit_s, bool query,
                    const double* origin, double radius);
  void livePostAll(long n_ticks, bool one_doorbell_per_tick);
  long liveDoneAll();
  // THE exception to the contract: liveWaitAll takes this list under the manager's lock and spins on it without (posts come
  // from other threads)
  std::vector<Batch*> liveOpenBatches();
  long liveStopAll();
  long rows() const;                    // slots of every batch
  void posesToDevice(double* out_dev);  // pose7 rows, batch after batch in slot order, on the shard's stream
  // the rows of the ids that this shard holds, grouped by batch (batch order), in the order of `ids` inside a batch
  void logCollect(const std::vector<unsigned>& ids, std::vector<LogRow>& rows);
  // rank_of_slot of every batch from the ascending ids of the WHOLE manager, uploaded to the shard's device / one
  // outputs_rows_kernel launch per batch with them
  void uploadRanks(const std::vector<unsigned>& sorted_all);
  void launchRows(double* pose_out);

 private:
  using Loc = TargetLoc;
  // lanes code of a new target's batch: the manager's explicit choice, or (auto) the axis-separable
  // layout when Q, R and every P0 allow it
  int chooseLayout(int type, const double* Q, const double* R, const double* P0, long n_P0) const;
  // the batch of (model, layout) -- created on first use -- and the parameter class of (Q, R) inside it
  int findOrCreateBatch(int type, const double* Q, const double* R, int lanes_code, int& cls);
  bool find(unsigned id, Loc& loc) const { return targets_.find(id, loc); }
  // ids of a host-array call by batch: sp.src[b] = their positions in the caller's arrays, slots[b] = their slots, both in
  // the caller's order; before_each(b, loc) runs ahead of every known id's entry (updateBatch's repeated-id flush)
  struct BySlot { Split sp; std::vector<std::vector<int>> slots; long known = 0; };
  template <class Before>
  void splitBySlot(const unsigned* ids, long n, BySlot& by, Before&& before_each) const;
  Batch* wholeBatch(const unsigned* ids, long n) const;   // the batch whose ids, in slot order, are exactly these; or null
  void notFound(unsigned id) const;   // "Target(id) does not exist!"

  const ShardSettings& set_;
  std::mutex* const owner_lock_;
  IdTable targets_;   // id -> (batch, slot); the reference's std::map<unsigned, TargetPtr> (target_manager.hpp:201)
  std::vector<std::unique_ptr<Batch>> batches_;
  hipStream_t stream_ = nullptr;

  // recorded all-batches sequences (stepSequenceAll): 8 kept, stamped when they are made only, so the oldest one goes
  struct SeqKey {
    long n_ticks; DtKey dt; bool query; double origin[3]; double radius;
    std::vector<Batch::SeqSpec> specs;
    std::vector<Batch::DevIdentity> ident;
  };
  SeqGraphCache<SeqKey> seq_graphs_{8};
  // (declaration order matters from here on: the streams and events are declared ahead of the buffers used on them, so the
  // buffers, destroyed last to first, go before them)
  std::vector<Stream> branch_streams_;   // [0]: the capture stream
  std::vector<Event> branch_events_;
  void dropSeqGraphs() { seq_graphs_.drop(); }
  void enqueuePopulationTick(hipStream_t st, long s, double dt, const Batch::SeqSpec* specs, bool query, const double* origin, double radius,
                             bool reverse, bool ab);
  FusedAllRoute fusedAllRoute(const Batch::SeqSpec* specs, bool scheduled, long n_ticks) const;
  DtTableRing dttab_;   // the time-step table of stepFusedAll's one launch: one table serves all parts (dt_table_ring.hpp)
  bool seq_flip_ = false;   // zig-zag across the whole tick: the next eager all-batches tick runs last batch first, tiles backwards
  // the scratch of the selections of this shard and of its batches (Batch::set_soonest_scratch): allocated at the first selection,
  // released through device_free
  SoonestScratch soonest_;
  AssocScratch assoc_;   // ... and of its associations (Batch::set_assoc_scratch): grow-only
  LifecycleScratch life_;   // ... and of its lifecycle calls: grow-only
  MergeScratch merge_;      // ... and of its duplicate searches: grow-only
  void mergeSearch(double dt, double gate, long rounds, double cell, int min_hits, const MergeSlotOut* out, int* info_dev);
  int soonestParts(const SoonestSpec* specs, long n_specs, int first_batch, SoonestPart* parts) const;

  // device-side id resolution for the array-of-ids calls (id_resolve.hpp): the table and the staging of one call
  struct DevIds {
    DeviceBuf<unsigned> keys, vals; DeviceBuf<int> seen;
    int log2cap = 0; bool dirty = true; int epoch = 0;
    long cap = 0;                       // entries the staging holds
    DeviceBuf<unsigned> ids; DeviceBuf<int> loc, idx;
    DeviceBuf<double> aos; DeviceBuf<char> soa; DeviceBuf<unsigned char> mask, found;
    DeviceBuf<double> out;              // [cap][7 + 6 + 6] getter outputs
    DeviceBuf<double> gnis; DeviceBuf<unsigned char> gev;   // [cap] the update policy's rows by entry
    DeviceBuf<ResolveCounters> counters;
    PinnedBuf<ResolveCounters> h_counters;
  } dev_ids_;
  static constexpr long kDevResolveMin = 8192;   // below this the host table is faster than the extra launches
  bool smallBatchPath(long n) const;
  void devIdsReserve(long n);
  void devIdsRebuild();
  // loc[e] of every id on the device + the per-batch counts on the host; false: not applicable (too many batches)
  bool resolveOnDevice(const unsigned* ids, long n, ResolveCounters& out);

  // per batch: rank_of_slot on the batch's device (getEstAllById), rebuilt after a change of membership
  struct RankMap { Event copied; DeviceBuf<int> dev; PinnedBuf<int> host; long cap = 0; };   // host: pinned staging
  std::vector<RankMap> rank_maps_;
};

}  // namespace te
