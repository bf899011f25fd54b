// target_manager.hpp -- host-side mirror of the reference's TargetManager
// (include/target_estimation/target_manager.hpp:33-203) over device-resident batches.
//
// Same method names, argument meaning, return values and messages as the reference; Eigen types
// are replaced by raw arrays (the reference's Eigen-typed header needs Eigen3, absent here):
//   Vector7d pose/meas  -> const double[7]  [x y z qx qy qz qw]   (target_manager.hpp:60)
//   Vector6d twist/acc  -> const double[6]
//   MatrixXd Q, R, P0   -> row-major const double[n*n] / [m*m]
// Differences, all deliberate:
//   * targets live in HBM, grouped into one Batch per (model, Q, R); the id -> (batch, slot)
//     map is a hash table (id_table.hpp) and enumeration sorts, so it stays ascending by id as
//     with the reference's std::map;
//   * the per-target constructor dump (printInfo, target_interface.cpp:57-78) and the per-target
//     type line (target_manager.cpp:161-173) are printed only when verbose (env
//     TARGET_ESTIMATION_VERBOSE=1): a million-target init must not write a million dumps;
//   * every filter step runs on the GPU; there is no CPU path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <functional>
#include <unordered_map>
#include <utility>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "shard.hpp"
#include "shard_map.hpp"

namespace te {

// makes `dev` the calling thread's current HIP device for the guard's lifetime and restores the previous one (every call into
// a shard of a manager whose devices were named: Batch reads the current device).  dev < 0: does nothing.
struct DeviceGuard {
  int prev = -1, dev;
  explicit DeviceGuard(int d) : dev(d) { if (d >= 0) enter(); }
  ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  void enter();
};

class TargetManager {
 public:
  typedef std::shared_ptr<TargetManager> Ptr;
  // target_manager.hpp:38
  enum target_t { ANGULAR_RATES = 0, ANGULAR_VELOCITIES, UNIFORM_ACCELERATION, UNIFORM_VELOCITY };

  explicit TargetManager(int dtype = F64, int lanes_per_target = 0);
  // throws const char* "TargetManager default constructor failed!" like target_manager.cpp:111-118
  explicit TargetManager(const std::string& file, int dtype = F64, int lanes_per_target = 0);
  virtual ~TargetManager();

  // target_manager.cpp:135-142 (defaults from the YAML file; throws const char* if none loaded)
  void init(unsigned id, double dt0, double t0, const double* p0, const double* v0 = nullptr, const double* a0 = nullptr);
  // target_manager.cpp:144-179
  void init(target_t type, unsigned id, double dt0, double t0, const double* Q, const double* R, const double* P0,
            const double* p0, const double* v0 = nullptr, const double* a0 = nullptr);
  // target_manager.cpp:181-188
  void init(const std::string& file, unsigned id, double dt0, double t0, const double* p0, const double* v0 = nullptr,
            const double* a0 = nullptr);
  bool update(unsigned id, double dt, const double* meas);  // target_manager.cpp:190-202
  bool update(unsigned id, double dt);                      // :204-218
  virtual void update(double dt);                           // :220-225
  bool erase(unsigned id);                                  // :227-241
  bool getTargetPose(unsigned id, double* pose7);           // :252-261
  bool getTargetTwist(unsigned id, double* twist6);         // :263-272
  bool getTargetAcceleration(unsigned id, double* acc6);    // :274-283
  long long getNumberMeasurements(unsigned id);             // :285-295
  int getRejectionRun(unsigned id);   // consecutive gate rejections kept by the ..._reacquire calls; -1: unknown id
  // :120-124.  The reference publishes five channels per target through rt_logger (an external ROS package):
  // measurement (measured_pose_), pose (pose_internal_ = [xyz rpy]), twist, acceleration, covariance (the full P),
  // target_interface.cpp:32-40,50-55.  Equivalent observability without ROS: with a log directory set (setLogDirectory
  // or env TARGET_ESTIMATION_LOG_DIR) every log() appends one row per SELECTED target to <dir>/
  //   time_<id>  meas_pose_<id>  est_pose_<id>  est_twist_<id>      the files the reference's test writes and its plot script
  //                                                                  loads (test/target_manager_test.cpp:164-168,
  //                                                                  matlab/plot_target_manager_test.m:9-13)
  //   pose_<id>  est_acc_<id>  covariance_<id>                       the remaining rt_logger channels ([xyz rpy]; acc6; P row-major)
  // in writeTxtFile's text format (utils.hpp:96-120: values separated by one space, one row per line).  Selected =
  // setLogTargets(ids), or every target while the manager holds at most kLogAutoSelect of them; the files stay open
  // between calls and each gets ONE buffered write per call.  A larger population without a selection gets one file per
  // channel, <channel>_all, rows prefixed by the id -- one write per channel per call.  Without a directory: a no-op, as
  // the reference without LOGGER_ON.  Setting a directory switches the measured-pose rows on (setKeepMeasurement).
  void log();
  void setLogDirectory(const std::string& dir);
  void setLogTargets(const unsigned* ids, long n);   // n == 0: back to the automatic selection
  static constexpr long kLogAutoSelect = 64;
  // TargetInterface::getMeasuredPose (target_interface.cpp:117-121): kept only on request (measured_pose.hpp)
  void setKeepMeasurement(bool on);
  bool keepMeasurement() const { return settings_.keep_meas; }
  // May the fp64 batches this manager creates use the shared-axes storage form (batch_store.hpp)?  Default: yes unless
  // TE_SHARED_AXES=0.  Batches that exist keep their form, so set it before the first init; throws once there is a batch.
  void setSharedAxes(bool on);
  bool sharedAxes() const { return settings_.shared_axes; }
  // May its shared-axes batches keep uniform tiles (batch_store.hpp)?  Default: yes unless TE_UNIFORM_TILES=0.  As setSharedAxes:
  // before the first init; throws once there is a batch.
  void setUniformTiles(bool on);
  bool uniformTiles() const { return settings_.uniform_tiles; }
  bool getTargetMeasuredPose(unsigned id, double* pose7);          // false: unknown id or not kept
  // TargetInterface::getPeriodEstimate (target_interface.cpp:80-87): 2 pi / |omega| of the current twist, -1 if not rotating
  bool getTargetPeriodEstimate(unsigned id, double& period);
  // TargetInterface::getEstimatedTransform (target_interface.cpp:95-98): T_ as a row-major 4x4 [R t; 0 1]
  bool getTargetTransform(unsigned id, double* T16);
  // getN() / getM() (target_interface.hpp:142,148)
  bool getTargetDims(unsigned id, int& n, int& m);
  // getTarget(id)->getEstimator()->getQ() / getR() / getP0() (kalman.hpp:74-89), row-major doubles as given at init;
  // any pointer may be null.  false: unknown id (or, for P0 only, more distinct P0 matrices than the host mirror keeps)
  bool getTargetModelMatrices(unsigned id, double* Q, double* R, double* P0);
  std::vector<unsigned> getAvailableTargets();              // :126-133
  bool selectTargetType(const std::string& type_str, target_t& type);  // :52-65

  // TargetInterface getters reached through getTarget(id)-> in the reference
  bool getTargetPoseAt(unsigned id, double t1, double* pose7);      // getEstimatedPose(t)
  bool getTargetTwistAt(unsigned id, double t1, double* twist6);    // getEstimatedTwist(t)
  bool getTargetAccelerationAt(unsigned id, double t1, double* a6); // getEstimatedAcceleration(t)
  bool getTargetTime(unsigned id, double& t);                       // getTime()
  // getTarget(id)->getEstimator()->getState()/getP() (kalman.hpp:69-89); x [n], P [n*n] row-major
  int getTargetState(unsigned id, double* x, double* P);
  bool hasTarget(unsigned id);
  size_t size();

  // ---- batched extension (not in the reference) ----------------------------------------------
  long initBatch(const unsigned* ids, long n, double dt0, double t0, const double* p0, const double* v0, const double* a0);
  long initBatch(target_t type, const unsigned* ids, long n, double dt0, double t0, const double* Q, const double* R,
                 const double* P0, bool per_target_P0, const double* p0, const double* v0, const double* a0);
  // n targets whose (Q, R, P0) come from a table of n_classes parameter sets: class_of[i] is the row of target i
  // (the reference's init takes Q, R, P0 per target, target_manager.hpp:85-87; a table + index is the same thing
  // without n copies).  All classes of one layout share ONE batch, i.e. one launch per tick.
  long initBatchClasses(target_t type, const unsigned* ids, long n, double dt0, double t0, long n_classes, const double* Q,
                        const double* R, const double* P0, const unsigned* class_of, const double* p0, const double* v0,
                        const double* a0);
  // nis_out / event_out [n] (or null): the update policy's reports per entry, in the caller's order (target_manager_c.h,
  // target_manager_update_meas_batch_gated); a policy that a touched batch cannot serve throws before anything is stepped
  long updateBatch(const unsigned* ids, long n, double dt, const double* meas, const unsigned char* has_meas, double* nis_out = nullptr,
                   unsigned char* event_out = nullptr);
  // THE UPDATE POLICY of the by-id paths (reacquire_plan.hpp UpdateGate; Batch): sticky, per model type (-1: every model), off by
  // default, inherited by the batches created later.  Setting it flushes every queued one-target step first.  Throws
  // std::invalid_argument for a policy that is refused whatever the batch.
  void setUpdateGate(int type, double nis_max, int max_rejects);
  bool getUpdateGate(int type, double& nis_max, int& max_rejects);   // false: no such model type
  int updateGateServed(int type);   // 1 / 0: by-id updates of the model's batches would be served under a policy; -1: unknown (no batch)
  // erase many targets in one call (one compaction launch per batch); unknown or repeated ids are reported
  // like erase() does and skipped; returns the number erased
  long eraseBatch(const unsigned* ids, long n);
  long getPoseBatch(const unsigned* ids, long n, double* pose, double* twist, double* acc, unsigned char* found,
                    bool at_time = false, double t1 = 0.0);
  long getStateBatch(const unsigned* ids, long n, double* x, double* P);
  // IntersectionSolver::getIntersectionTimeWithSphere (src/intersection_solver.cpp:42-89): time from
  // t1 to the first crossing of the sphere, -1 if none or unknown id.
  double getIntersectionTimeWithSphere(unsigned id, double t1, const double* origin, double radius);
  // IntersectionSolver::getIntersectionPoseWithSphere without its moving-average convergence gate
  // (src/intersection_solver.cpp:91-104): true if an intersection exists; pose7 = pose at t1+delta.
  bool getIntersectionPoseWithSphere(unsigned id, double t1, const double* origin, double radius, double* pose7,
                                     double* delta = nullptr);
  // IntersectionSolver::getIntersectionPoseWithSphere with its convergence gate, same argument order
  // (intersection_solver.hpp:98-101); one gate per target (the reference has one per solver object).
  // Returns whether the filtered position / angle errors are below the thresholds.
  bool getIntersectionPoseWithSphere(unsigned id, double t1, double pos_th, double ang_th, const double* origin,
                                     double radius, double* pose7);
  void setIntersectionFiltersLength(int n) { settings_.filters_length = n; }   // IntersectionSolver ctor, default 250
  long intersectGatedBatch(const unsigned* ids, long n, double t1, double pos_th, double ang_th, const double* origin,
                           double radius, double* delta, double* pose, unsigned char* converged, unsigned char* found,
                           double* filt = nullptr);
  long intersectBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, double* delta,
                      double* pose, unsigned char* found);

  // n_ticks ticks of EVERY batch (specs in batch order), device-resident inputs: one step launch per
  // batch per tick, optionally followed by the own-time sphere query of every target.  The batches are
  // independent, so with use_graph != 0 each batch's chain of launches is its own branch of one hipGraph
  // and the branches run concurrently; the query runs inside the step kernel (QUERY variants).
  // use_graph == 2 records without launching.  use_graph == 0 issues the same launches eagerly, batch after batch per tick.
  bool populationTickNow();
  // sched: the call's time-step schedule (dt_schedule.hpp; by default none): tick s of every batch of every shard runs with
  // sched.dt[s], `dt` is not read, every batch's clock advances tick by tick.
  void stepSequenceAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, bool query,
                       const double* origin, double radius, int use_graph, const DtSchedule& sched = DtSchedule{});
  // The same with a per-tick pose stream per batch (poses[b], PoseStream; one with a null dev writes nothing for that batch):
  // written by the step kernels -- the population kernel's POSE variant where the tick is one launch -- or by a pose-writer
  // launch behind each tick of a batch whose layout has no POSE kernel.  Every stream is checked before anything is enqueued.
  // innov (or null): a per-tick innovation stream per batch as well (innov[b], InnovStream; one with a null nis writes nothing for
  // that batch), routed like the pose streams: the step kernels' INNOV variants -- the population kernel's where the tick is one
  // launch -- or an innovation-writer launch ahead of each tick of a batch whose layout has none.
  void stepSequenceAll(long n_ticks, double dt, const Batch::SeqSpec* specs, const PoseStream* poses, long n_specs, bool query,
                       const double* origin, double radius, int use_graph, const InnovStream* innov = nullptr,
                       const DtSchedule& sched = DtSchedule{});

  // A temporally fused replay of EVERY batch (specs in batch order, shard-major; poses and innov inside the specs): for every batch
  // what Batch::step_fused_gated leaves, bit for bit, with one launch per shard where Shard::stepFusedAll says so.  Every refusal is
  // made before any batch of any shard is changed.
  void stepFusedAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, const DtSchedule& sched = DtSchedule{});
  int fusedAllServed(bool gated, bool scheduled);   // 1: one launch per shard that holds targets; 0: per batch

  // THE k SOONEST CROSSINGS of the whole manager (select_soonest.hpp; target_manager_select_soonest[_dev]): specs [numBatches()]
  // in batch order, shard-major (a spec without delta skips its batch).  Candidates: (ok == null || ok[i]) && lo <= delta[i] <= hi;
  // order: (delta, batch index, slot).  Per shard all its batches are selected together by one set of launches on the shard's
  // stream; the shards' <= k rows each are merged on the host (merge_soonest).  Everything is checked before anything is enqueued
  // on any shard.  No record is read: no tile is settled, no batch demoted, no recording dropped.  rows [k]; ids [k] from the
  // batches' slot -> id tables ((unsigned)-1 in a filler row).  Returns count.
  long selectSoonest(const SoonestSpec* specs, long n_specs, double lo, double hi, long k, bool with_pose, SoonestRow* rows, unsigned* ids);
  // the same into device memory, without a host wait: a manager on one device only (several have no single device to write to)
  void selectSoonestDev(const SoonestSpec* specs, long n_specs, double lo, double hi, long k, const SoonestOut& out);

  // POSITION COVARIANCE AND TIME SPREAD AT THE CROSSINGS (crossing_cov.hpp; target_manager_crossing_cov_dev / _batch).
  // crossingCovDev: for the rows selectSoonestDev left on the device (batch / slots / delta [n <= kCrossingCovMaxRows]); a manager
  // on one device only.  crossingCovBatch: by id with host arrays, over every shard; the queued one-target steps run first; unknown
  // ids get the filler; returns the ids found.  Neither settles a tile, demotes a batch, drops a recording or touches a clock.
  void crossingCovDev(double t1, const double* origin, double radius, const int* batch_dev, const int* slots_dev, const double* delta_dev,
                      long n, double sigma_r_max, double sigma_t_max, double* cov_dev, double* sigma_dev, unsigned char* ok_dev);
  long crossingCovBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, const double* delta,
                        double sigma_r_max, double sigma_t_max, double* cov, double* sigma, unsigned char* ok);

  // ASSOCIATION OF UNLABELLED DETECTIONS with every target of the manager (associate.hpp; target_manager_associate[_dev]): out
  // [numBatches()] in target_manager_get_batch order; a manager on one device only.  associateDev: no host wait; associate: host
  // detections in, per-detection rows with ids back, returns the matched count.  Neither settles a tile, demotes a batch, drops a
  // recording or touches a clock; the queued one-target steps run first.
  // grid_cell > 0: the grid form (associate_grid.hpp; target_manager_associate_grid[_dev]), 0: the brute-force form.
  void associateDev(double dt, const double* det_dev, long M, double gate, long rounds, const AssocSlotOut* out, long n_out,
                    int* slot_of_det_dev, int* batch_of_det_dev, double* d2_of_det_dev, int* info_dev, double grid_cell = 0.0);
  long associate(double dt, const double* det, long M, double gate, long rounds, const AssocSlotOut* out, long n_out, unsigned* ids_of_det,
                 int* batch_of_det, int* slot_of_det, double* d2_of_det, long* unmatched, long* n_unmatched, int* info, double grid_cell = 0.0);

  // THE TRACK LIFECYCLE (lifecycle.hpp; target_manager_lifecycle), run after the tick that consumed an association:
  // retires the targets that went max_misses frames without a match and creates one from every unmatched finite detection, on the
  // device (Shard::lifecycle says how).  has_dev [n_masks] in target_manager_get_batch order; a manager on one device only.  A policy
  // without Q, R, P0 means the manager's own model parameters and is refused unless birth_type is the manager's default model.
  // Every refusal leaves counters, records, ids and sizes as they were.
  void lifecycle(const double* det_dev, const int* slot_of_det_dev, long M, const unsigned char* const* has_dev, long n_masks,
                 const LifecyclePolicy& policy, unsigned* retired_ids_out, long retired_cap, long* info);
  // DUPLICATE TRACKS (track_merge.hpp; target_manager_find_duplicates_dev / target_manager_retire_duplicates): two
  // tracks that follow the same object, found by a self-join through the association's grid (Shard::findDuplicatesDev /
  // retireDuplicates say how); a manager on one device only.  retireDuplicates closes the log files of the targets that went away.
  void findDuplicatesDev(double dt, double gate, long rounds, double cell, int min_hits, const MergeSlotOut* out, long n_out, int* info_dev);
  void retireDuplicates(double dt, double gate, long rounds, double cell, int min_hits, unsigned* retired_ids_out, unsigned* kept_ids_out,
                        long cap, long* info);
  bool getTrackCounts(unsigned id, int& miss, int& hits);   // false: unknown id

  // Resident ("live") mode for EVERY batch of the manager at once (Batch::live_start per batch, each kernel on its own
  // stream so that they are resident together): BASELINE configs[3] / configs[4] put two motion models on every GPU, and
  // their per-GPU share (62 500 + 62 500 targets) is launch-bound.  specs as for stepSequenceAll (ring_ticks > 0 required).
  // The wavefronts of all sessions must fit the device together: sum over batches of waves / capacity <= 1.
  // query: also the own-time sphere query of every target after every tick into specs[b].delta_dev / pose_dev (configs[4])
  void liveStartAll(double dt, const Batch::SeqSpec* specs, long n_specs, long first_entry, long max_ticks, double idle_limit_s,
                    bool query = false, const double* origin = nullptr, double radius = 0.0);
  void livePostAll(long n_ticks, bool one_doorbell_per_tick);
  long liveDoneAll();                       // ticks every wavefront of every batch has finished
  bool liveWaitAll(long tick, double timeout_s);
  long liveStopAll();                       // returns the ticks served (the same for every batch)
  // batches of every shard, shard-major (a manager on one device: its own batches)
  int numBatches() const;
  Batch* batch(int i);
  Batch* batchOfType(int type);
  void setStream(hipStream_t s);   // refused on a manager with more than one shard (setShardStream)
  hipStream_t stream() const { return several() ? nullptr : shards_[0]->stream(); }

  // ---- several devices (target_manager_set_devices) ----
  // n shards (shard.hpp), shard k on HIP device devices[k] (repeats allowed).  Only before the first target; n == 1 on the
  // creation device is the manager as constructed.  Throws and leaves the manager unchanged otherwise.
  void setDevices(const int* devices, int n);
  int numShards() const { return (int)shards_.size(); }
  int shardDevice(int k) const;      // -1: no such shard
  int shardOf(unsigned id);          // -1: unknown id
  int batchShard(int i) const;       // shard of batch i (numBatches order), -1: no such batch
  void setShardStream(int k, hipStream_t s);
  // pose7 of every target in ascending id order (getAvailableTargets) into pose_out [size()][7] (device memory every shard's
  // device reaches, or pinned host memory); one outputs_rows_kernel launch per batch, asynchronous (complete at synchronize()).
  // After a change of membership the row maps are rebuilt on the host; a map that grows waits for its batch's stream.
  // pose_out == null only counts.  Returns the number of rows.
  long getEstAllById(double* pose_out, long capacity);
  // pose7 rows (doubles) of every target, batch after batch in slot order, into out_dev [size()][7] on stream `st`
  // (the gather's send side, pose_gather.hpp); out_dev == null only counts.  Returns the number of rows.
  long posesToDevice(double* out_dev, long capacity, hipStream_t st);
  // The gather's enqueue step, atomic with respect to init / erase / setStream: under the manager's lock, checks that the
  // manager holds expect_rows rows, calls prepare(rows, stream) -- which may enqueue waits on that stream and returns the
  // destination [rows][7] -- and launches the outputs kernels into it.  Returns the row count.
  long posesForGather(long expect_rows, const std::function<double*(long, hipStream_t)>& prepare);
  void synchronize();
  int dtype() const { return settings_.dtype; }
  bool defaultsLoaded() const { return default_values_loaded_; }
  int defaultType() const { return (int)default_type_; }

 protected:
  bool loadYamlFile(const std::string& file, std::vector<double>& Q, std::vector<double>& R, std::vector<double>& P,
                    target_t& type);  // target_manager.cpp:67-104

 private:
  std::mutex target_lock_;   // THE lock: every public method takes it once; shards and batches have none of their own
  ShardSettings settings_;   // what the shards read (shard.hpp)
  std::vector<double> default_Q_, default_P_, default_R_;
  target_t default_type_ = UNIFORM_VELOCITY;
  bool default_values_loaded_ = false;

  // ---- shards.  Never empty: without setDevices one shard on the device current at construction, and then no DeviceGuard
  // and no ShardMap (the shard's own id table answers).  With setDevices: shard k on shard_dev_[k] under a DeviceGuard, and
  // with more than one shard the ShardMap says which shard holds an id.
  std::vector<std::unique_ptr<Shard>> shards_;
  std::vector<int> shard_dev_;
  bool placed_ = false;     // setDevices named the devices
  int home_dev_ = 0;        // the device current at construction
  ShardMap shard_map_;      // more than one shard only
  bool ranks_dirty_ = true; // membership changed since the row maps of getEstAllById were uploaded
  // (model, layout) of the shards' batches in order of first creation: the batch order one shard would have (log()); more than one shard only
  std::vector<std::pair<int, int>> batch_keys_;
  void noteBatchKeys();
  bool several() const { return shards_.size() > 1; }
  int guardDev(size_t k) const { return placed_ ? shard_dev_[k] : -1; }   // what a DeviceGuard around a call into shard k takes
  size_t count() const { return several() ? shard_map_.size() : shards_[0]->size(); }
  std::vector<unsigned> sortedIds() const;
  // the shard that answers for id (shard 0 for an id that no shard holds: it answers as a manager on one device does)
  size_t shardFor(unsigned id) const {
    if (!several()) return 0;
    const int k = shard_map_.shard_of(id);
    return k < 0 ? 0 : (size_t)k;
  }
  // THE routing point of the by-id calls: lock, the id's shard made current, f(shard).  (Always inline, like getOne: left
  // to itself the compiler calls the instantiation through the PLT, which the one-target cycle pays per call.)
  template <class F>
  __attribute__((always_inline)) auto routeId(unsigned id, F&& f) -> decltype(f(std::declval<Shard&>())) {
    std::lock_guard<std::mutex> lg(target_lock_);
    const size_t k = shardFor(id);
    DeviceGuard g(guardDev(k));
    return f(*shards_[k]);
  }
  // THE routing point of the host-array calls (caller holds target_lock_): the ids by shard (row_split.hpp), then
  // f(shard, k, its ids, how many, pos) for every shard that holds some, made current; pos = their positions in the caller's
  // arrays.  One shard takes the call whole: no split, the caller's ids and pos == null.
  Split splitIds(const unsigned* ids, long n) const;
  template <class F>
  void forShards(const Split& sp, const unsigned* ids, long n, F&& f) {
    if (!several()) {
      DeviceGuard g(guardDev(0));
      f(*shards_[0], (size_t)0, ids, n, (const std::vector<long>*)nullptr);
      return;
    }
    for (size_t k = 0; k < shards_.size(); ++k) {
      if (sp.src[k].empty()) continue;
      const std::vector<unsigned> ids2 = gatherRows(ids, sp.src[k], 1);
      DeviceGuard g(guardDev(k));
      f(*shards_[k], k, ids2.data(), (long)ids2.size(), &sp.src[k]);
    }
  }
  // THE refusal, for the calls that need the manager to be one shard (live mode, gather, setStream): lock, the check, the
  // shard made current, f(shard)
  void requireOneShard(const char* what) const;
  template <class F>
  auto onlyShard(const char* what, F&& f) -> decltype(f(std::declval<Shard&>())) {
    std::lock_guard<std::mutex> lg(target_lock_);
    requireOneShard(what);
    DeviceGuard g(guardDev(0));
    return f(*shards_[0]);
  }
  __attribute__((always_inline)) bool getOne(unsigned id, double* pose7, double* twist6, double* acc6, bool at_time, double t1) {   // the six one-target getters
    return routeId(id, [&](Shard& s) { return s.outputsOne(id, pose7, twist6, acc6, at_time, t1); });
  }
  long createBatch(target_t type, const unsigned* ids, long n, double t0, const double* Q, const double* R, const double* P0,
                   bool per_target_P0, const double* p0, const double* v0, const double* a0, long n_classes, const unsigned* class_of);

  // ---- log()
  std::string log_dir_;
  std::vector<unsigned> log_ids_;                       // explicit selection (sorted); empty = automatic
  struct LogFiles { std::FILE* f[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; };
  std::unordered_map<unsigned, LogFiles> log_files_;    // per selected target, kept open
  std::FILE* log_all_[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  void closeLogFiles();
  void closeLogFilesOf(unsigned id);
  void logWrite(const std::vector<LogRow>& rows, bool per_target);
};

}  // namespace te
