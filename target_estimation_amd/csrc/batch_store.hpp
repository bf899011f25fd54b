// batch_store.hpp -- device-resident store of all targets of one motion model / parameter set /
// precision, and the launches that act on it.  Replaces, for N targets at once, the per-target
// objects of the reference (TargetInterface + its KalmanFilterInterface:
// include/target_estimation/target_interface.hpp:193-282, kalman.hpp:95-150): instead of
// (x, P, A, C, Q, R, P0, K, I) per target there is one shared (Q, R) and one lane record
// (x, P, unwrap memory) per target in HBM (te_layout.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "dev_mem.hpp"
#include "dt_schedule.hpp"
#include "dt_table_ring.hpp"
#include "kf_ops.hpp"
#include "reacquire_plan.hpp"
#include "seq_graph_cache.hpp"
#include "select_soonest.hpp"
#include "crossing_cov.hpp"
#include "associate.hpp"
#include "associate_grid.hpp"
#include "lifecycle.hpp"

namespace te {

// A per-tick pose stream (target_pose_stream_c): after tick s of a call, the estimated pose of every slot (getEstimatedPose, as
// outputs_dev derives it), doubles SoA [7][ld] with column = slot, in block b = (ring > 0 ? s % ring : s) at dev + b * tick_stride
// (tick_stride 0: every tick overwrites one block).  dev == null: no poses.
struct PoseStream {
  double* dev = nullptr;
  long ld = 0;
  long tick_stride = 0;
  long ring = 0;
  double* block(long s) const { return dev ? dev + (ring > 0 ? s % ring : s) * tick_stride : nullptr; }
  bool same(const PoseStream& o) const { return dev == o.dev && ld == o.ld && tick_stride == o.tick_stride && ring == o.ring; }
};

// A per-tick innovation stream (target_innov_stream_c): after tick s of a call, for every slot (column), the tick's normalised
// innovation squared nu^T S^-1 nu in row b = (ring > 0 ? s % ring : s) of nis (rows nis_tick_stride apart) and, unless innov is null,
// its innovation nu = y - x^-[0:m] in block b of innov, SoA [m][ld] (blocks innov_tick_stride apart); a stride of 0 overwrites one
// row / block every tick.  A slot without a measurement on the tick: NIS = -1, nu = 0.  nis == null: no stream.
struct InnovStream {
  double* nis = nullptr;
  double* innov = nullptr;
  long ld = 0;
  long nis_tick_stride = 0;
  long innov_tick_stride = 0;
  long ring = 0;
  // The validation gate that goes with the stream (StepParams::gate): > 0 (+inf included) = a measurement is folded in iff its
  // (double)NIS <= gate, a rejected one leaves the target as a tick without a measurement would; the stream reports NIS and nu of
  // every measured slot, so the decision is 0 <= nis <= gate.  0: none.  Needs the NIS row.
  double gate = 0.0;
  bool gated() const { return gate > 0.0; }
  // The re-acquisition policy that goes with the gate (reacquire_plan.hpp; target_reacquire_c): rejection runs, event rows,
  // re-initialisation on the K-th consecutive rejection.  Off by default.
  Reacquire reacq{};
  bool on() const { return nis != nullptr; }
  bool plain() const { return !on() && !gated() && !reacq.on; }   // no stream, no gate, no policy
  double* nis_row(long s) const { return nis ? nis + (ring > 0 ? s % ring : s) * nis_tick_stride : nullptr; }
  double* innov_block(long s) const { return (nis && innov) ? innov + (ring > 0 ? s % ring : s) * innov_tick_stride : nullptr; }
  bool same(const InnovStream& o) const {
    return nis == o.nis && innov == o.innov && ld == o.ld && nis_tick_stride == o.nis_tick_stride && innov_tick_stride == o.innov_tick_stride && ring == o.ring &&
           gate == o.gate && reacq.same(o.reacq);   // (recorded graphs are keyed by the gate and the re-acquisition policy as well)
  }
};

class Batch {
 public:
  // `owner_lock`: the one mutex of the manager whose shard owns the batch (TargetManager::target_lock_, whatever the number
  // of shards); the C boundary takes it around every call made through a batch handle, so that those calls and the
  // manager's own are serialised
  // allow_shared: an fp64 batch in the separable layout with packed groups (lanes 301) whose Q and R allow it (te_layout.hpp,
  // shared_axes_qr_ok) starts in the shared-axes storage form: one covariance block per kind of axis instead of one per axis.
  // Same results bit for bit, fewer bytes per tick.  The batch leaves the form for good (demote_shared) when something arrives
  // that it does not serve; lanes_code() and layout().layout read 301 / 3 in both forms.
  // allow_uniform_tiles: a batch in that form whose kernels have the feature (LayoutInfo::lin_words) keeps uniform tiles, see below
  Batch(int type, int dtype, int lanes, const double* Q, const double* R, hipStream_t stream, std::mutex* owner_lock = nullptr,
        bool allow_shared = false, bool allow_uniform_tiles = true);
  ~Batch();
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;

  std::mutex* owner_lock() const { return owner_lock_; }
  int type() const { return type_; }
  int lanes_code() const { return lanes_code_; }
  int dtype() const { return dtype_; }
  int n_state() const { return ops_->L.n; }
  int n_meas() const { return ops_->L.m; }
  const LayoutInfo& layout() const { return ops_->L; }
  bool shared_axes() const { return ops_->L.shared_axes != 0; }
  // Expand a shared-axes batch to the plain records of its layout, once and for good: a new record buffer, every kind's block
  // copied to each of its axes (exact), the plain launch table from then on; recorded sequences are dropped.  Called by the batch
  // itself ahead of what the shared form does not serve: a second (Q, R) class, an initial covariance whose blocks differ between
  // the axes of a kind, step_fused, live_start, set_state.  No-op for a plain batch.
  void demote_shared();
  // UNIFORM TILES (te_layout.hpp Cfg::UT; kf_step.hpp StepArgs::tile_uni).  The linear P words of a chain are a function of the
  // block before the tick, Q, R, dt and the has-bit, so the targets of a tile that agree on them keep agreeing while they get the
  // same dt and has-bit -- a population created in bulk and measured every tick, tile after tile.  The dense step finds such
  // tiles itself (a launch with StepParams::promote compares the lanes' bits), keeps ONE copy of the words per tile in
  // d_tile_blk_ and neither loads nor stores the record's linear-covariance chunks of a flagged tile; it ends a tile's uniformity
  // itself on the tick whose has-bits split it.  Records + blocks + flags are the whole, current state after every tick.
  // Every launch that is not a dense tick of the form, get_state and an x-only reader must see plain records: it gets them
  // through records(), i.e. behind settle_tiles() -- one dense launch that writes each flagged tile's block back into its lanes
  // (an exact copy) and clears the flags; a no-op while no promoting launch has run since the last one.  Dense ticks promote only
  // after promote_after() consecutive ones since the last settle (default 2, env TE_UNIFORM_TILES_AFTER), so that a caller who
  // interleaves by-id updates with dense ticks never pays a settle pass per tick; recorded sequences always promote.
  bool uniform_tiles_enabled() const { return ut_on_ && ops_->L.lin_words > 0; }
  void settle_tiles();
  long uniform_tiles();        // tiles flagged now: reads the flags back on the batch's stream (SYNCHRONISES)
  static long promote_after();
  struct RecordingScope {   // while one lives, the dense ticks enqueued go into a recorded graph (they promote: a dense streak)
    Batch& b;
    explicit RecordingScope(Batch& x) : b(x) { b.recording_ = true; }
    ~RecordingScope() { b.recording_ = false; }
    RecordingScope(const RecordingScope&) = delete;
  };
  void note_replay(long n_ticks) { if (uniform_tiles_enabled()) { ut_flagged_ = true; dense_streak_ += n_ticks; } }   // a recorded sequence was launched
  long size() const { return n_; }
  bool getter_table_is_cheap() const { return n_ <= kCacheMax; }   // (its one-target getters read a host-resident table from the first call after a change)
  size_t elem_size() const { return dtype_ == F64 ? 8 : 4; }
  // Parameter classes: the (Q, R) pairs of the batch's targets (TargetManager::init takes them per target,
  // target_manager.hpp:85-87).  One class: Q, R are shared by every lane (scalar cache / LDS).  Several: a table in
  // HBM plus one class index per slot, and the per-class kernels (PERQR) -- still one launch per tick.
  int find_class(const double* Q, const double* R) const;   // -1: not there
  int add_class(const double* Q, const double* R);
  int n_classes() const { return n_classes_; }
  void set_stream(hipStream_t s) { stream_ = s; }
  hipStream_t stream() const { return stream_; }
  unsigned slot_id(long slot) const { return slot_ids_[slot]; }
  const std::vector<unsigned>& slot_ids() const { return slot_ids_; }
  double clock() const { return t_acc_.hi + t_acc_.lo; }

  // Construct `count` new targets in slots [size(), size()+count).  Host arrays.
  // cls: the class of every new target, or cls_of [count] one class each; P0_index [count] (with P0 = a table of
  // P0_count matrices) gives every target the initial covariance of its row of the table.
  long append(long count, const unsigned* ids, double t0, const double* P0, bool per_target_P0,
              const double* p0, const double* v0, const double* a0, int cls = 0, const int* cls_of = nullptr,
              const int* P0_index = nullptr, long P0_count = 0);
  // Remove a slot by moving the last slot into it; returns the id that now lives in `slot`
  // (or the erased id if it was the last one).
  unsigned erase_slot(long slot);
  // Erase many slots at once (distinct slots, any order): survivors from the tail fill the holes below
  // the new size in ONE launch.  moves_out lists (id, new slot) of every target that changed slot.
  void erase_slots(const int* slots, long k, std::vector<std::pair<unsigned, int>>& moves_out);

  // One tick over every target, device-resident inputs (the fast path).
  //   meas_dev: SoA [7][ld] in the batch precision, or null (predict only = TargetInterface::update)
  //   has_dev : per-slot mask or null (all have a measurement)
  void step_dense(double dt, const void* meas_dev, long ld, const unsigned char* has_dev);
  // n_ticks consecutive dense ticks, tick s reading meas_base + s * tick_stride (elements of the
  // batch precision) and has_base + s * has_stride: exactly n_ticks launches of the step kernel,
  // enqueued from C++ (use_graph 1: recorded once into a hipGraph and replayed, which removes the
  // per-launch host cost when a recorded stream is replayed; 2: record only, launch nothing).
  // poses: the per-tick pose stream of the call (PoseStream; by default none), written by the step kernel where the layout has a
  // POSE variant, by a pose-writer launch behind every tick otherwise (OpsImpl::step)
  // innov: the per-tick innovation stream of the call (InnovStream; by default none), written by the step kernel where the layout
  // has an INNOV variant, by an innovation-writer launch ahead of every tick otherwise (OpsImpl::step).  Its ticks run in place
  // (no A -> B variant) -- same bits.
  // sched: the call's time-step schedule (DtSchedule; by default none).  With one, tick s is launched with dt = sched.dt[s] and `dt`
  // is not read; the clock advances by one te_clock_add per tick, and a recording is filed under the schedule's bits.
  void step_sequence(long n_ticks, double dt, const void* meas_base, long tick_stride, long ld,
                     const unsigned char* has_base, long has_stride, int use_graph, long ring_ticks = 0,
                     const PoseStream& poses = PoseStream{}, const InnovStream& innov = InnovStream{}, const DtSchedule& sched = DtSchedule{});
  // n_ticks ticks in ONE launch: every target's state stays in registers across the ticks and only
  // the measurements are read per tick.  Same results as n_ticks single ticks; a different
  // ("effective", temporally fused) cost model -- for replaying recorded streams.
  // sched: the call's time-step schedule, or none (step_fused_gated below says who serves it).
  void step_fused(long n_ticks, double dt, const void* meas_base, long tick_stride, long ld,
                  const unsigned char* has_base, long has_stride, const PoseStream& poses = PoseStream{}, const DtSchedule& sched = DtSchedule{});
  // step_fused with the innovation stream, the validation gate and the re-acquisition policy of step_sequence INSIDE the fused call
  // (target_batch_step_fused_gated): per slot and tick, bit for bit, what step_sequence(..., use_graph 0, ring_ticks 0, poses, innov)
  // leaves -- state, covariance, unwrap memory, counter, clock, rejection runs, every NIS row, innovation block, event row and pose
  // block.  ONE launch for the whole call (kf_step_sep_fused_gate_kernel: the run in a register across the ticks, lost targets
  // re-initialised in registers) where fused_gate_served(); every other batch, and a call with a pose stream, runs the sequence's
  // ticks -- same results, its launch counts.  !innov.on(): exactly step_fused.  Refusals (invalid_argument, nothing launched): those
  // of step_sequence's streams, n_ticks beyond an int, negative strides, ld < size.  A shared-axes batch is expanded first.
  // sched: the call's time-step schedule (target_batch_step_fused_dt), or none.  With one, tick s of the call runs with sched.dt[s]: per
  // slot and tick, bit for bit, what the single ticks step_dense(sched.dt[s], ...) / step_sequence(1, sched.dt[s], ...) leave, the
  // clock included.  ONE launch where fused_dt_served(): the kFused loop, plain or gated, reading a device table the batch owns and
  // fills on its stream ahead of the launch (dt_table_push); everywhere else the single ticks -- same results.
  void step_fused_gated(long n_ticks, double dt, const void* meas_base, long tick_stride, long ld, const unsigned char* has_base,
                        long has_stride, const PoseStream& poses, const InnovStream& innov, const DtSchedule& sched = DtSchedule{});
  // one launch per fused call with a schedule (without a pose stream): gated = the call carries an innovation stream, a gate or a
  // policy (the gated loop), else the plain loop
  // (a shared-axes batch says no: its call is the expansion to the plain form, a synchronisation, and then that form's launch)
  bool fused_dt_served(bool gated) const {
    if (shared_axes()) return false;
    if (gated) return fused_gate_served() && ops_->fused_gate_dt != 0;
    return ops_->fused_dt != 0 && n_classes_ == 1 && !keep_meas_;
  }
  // one launch per fused gated call (without a pose stream): the plain form of this batch has the kernel, one (Q, R) class, no
  // measured-pose rows
  bool fused_gate_served() const {
    const Ops* o = shared_axes() ? get_ops(type_, dtype_, lanes_code_) : ops_;
    return o && o->fused_gate != 0 && n_classes_ == 1 && !keep_meas_;
  }
  // throws std::invalid_argument unless `poses` is none or a valid stream for this batch (ld >= size, tick_stride 0 or >= 7 ld,
  // ring >= 0): checked before a call enqueues anything
  void check_pose_stream(const PoseStream& poses) const;
  // the same for an innovation stream: ld >= size, nis_tick_stride 0 or >= ld, innov_tick_stride 0 or >= m ld, nothing negative
  // ... and, with it, the gate and the re-acquisition policy it carries (reacquire_plan.hpp, check_reacquire)
  // count_only_needs_no_p0: a policy with K = 0 is not refused on a batch that no longer keeps its initial covariances (the fused
  // gated kernel, like the resident one, reads none for it)
  void check_innov_stream(const InnovStream& innov, bool count_only_needs_no_p0 = false) const;
  // Before a call with a re-acquisition policy enqueues or records anything: bring the device copies of the initial-covariance
  // table and of the slot -> row index up to date (a table that had to grow drops the recorded sequences; dev_identity() shows it).
  void prepare_reacquire(const InnovStream& innov);
  // the rejection run of every slot (host array [size()]); synchronises
  void rejection_runs(unsigned char* out);
  int rejection_run(long slot);
  // THE TRACK COUNTERS (lifecycle_plan.hpp; target_manager_lifecycle): per slot the run of consecutive lifecycle
  // calls without a match (miss) and the calls with one since creation (hits), both saturating at 255.  Library-owned like the
  // rejection runs: 0 at creation, they follow their target through erase and growth; only the lifecycle's commit writes them.
  void track_counts(unsigned char* miss_out, unsigned char* hits_out);   // host arrays [size()]; synchronises
  void track_count(long slot, int& miss, int& hits);
  unsigned char* track_miss_dev() const { return d_miss_.get(); }
  unsigned char* track_hits_dev() const { return d_hits_.get(); }
  // `count` new targets whose poses are rows of a frame in DEVICE memory: p0 of target r = det_dev[rows_dev[r]] (seven doubles),
  // v0 = a0 = null, one P0 and class for all -- record for record what append(count, ids, t0, P0, false, p0, null, null, cls)
  // creates from the same rows, through the same init launcher; only the staging of p0 is a gather launch instead of a copy.
  long append_gathered(long count, const unsigned* ids, double t0, const double* P0, int cls, const double* det_dev, const int* rows_dev);
  // RESIDENT ("live") mode for small batches: ONE launch stays on the device with the batch's state in registers and serves
  // tick after tick as the host posts them -- no per-tick dispatch (a dependent launch costs 1.5-2 us, more than the tick of a
  // 10^4-target batch itself).  Protocol:
  //   live_start(dt, ring...)   launch; the ring (device memory, SoA ticks as for step_sequence) receives tick k's measurements
  //                             in entry (first_entry + k) % ring_ticks BEFORE tick k is posted
  //   live_post(n)              "n more ticks are in the ring": one store to a host-mapped word the wavefronts poll
  //   live_done()               ticks every wavefront has finished (one host-mapped word, kept by the kernel's relay wavefront)
  //   live_wait(tick, timeout)  spin until live_done() >= tick
  //   live_stop()               ask the kernel to finish the posted ticks, store the records and exit; accounts the ticks
  // Results are those of single ticks, bit for bit.  While a session is open the records in HBM are stale; every other call
  // on the batch (steps, getters, erase, ...) ends the session first.  The whole grid must be resident (the wavefronts wait
  // for the host, not for each other, but one that never starts would miss its ticks): refused beyond live_capacity().
  // A wavefront that sees no news for idle_limit_s gives up on its own (a dead host leaves no kernel behind).
  // q_delta_dev [size] (+ q_pose_dev [size][7] or null): also run the own-time sphere query of every target after every tick
  // (outputs overwritten every tick), as enqueue_tick's fused query does
  void live_start(double dt, const void* meas_ring, long tick_stride, long ld, const unsigned char* has_ring, long has_stride,
                  long ring_ticks, long first_entry, long max_ticks, double idle_limit_s, const double* q_origin = nullptr,
                  double q_radius = 0.0, double* q_delta_dev = nullptr, double* q_pose_dev = nullptr);
  // pose_soa_dev [7][ld] doubles (device memory; null switches it off): the sessions started AFTER this call also write the
  // estimated pose of every target after every tick there (the reference's node publishes them every tick,
  // src/target_manager_ros.cpp:78-87), through the caches and before the tick counts as done -- a consumer that copies the
  // buffer on another stream after live_done() reached tick k reads the poses of a tick >= k (of tick k if it posts one tick at a time)
  void live_set_pose_output(double* pose_soa_dev, long ld);
  // THE GATE INSIDE THE SESSIONS started AFTER this call (target_batch_live_set_gate; kf_step_sep.hpp, LiveGate): g.gate > 0 with
  // the NIS rows of the session (g.nis; no innovation block) and, or not, the policy g.reacq -- the semantics per slot and tick of
  // step_sequence with the same stream, decided inside the resident kernel.  Tick k of a session writes NIS row and event row
  // k (or k % ring) through the caches, ahead of the tick's progress word.  The rejection runs are read when a session starts and
  // written back with its records.  !g.gated(): off.  Refusals throw and change nothing; live_gate_refusal says why this batch
  // cannot serve a gate at all (no resident kernel, several (Q, R) classes, measured-pose rows), or null.
  void live_set_gate(const InnovStream& g);
  const char* live_gate_refusal() const;
  bool live_gate_set() const { return live_.gate.gated(); }
  void live_post(long n_ticks);
  long live_done() const;
  bool live_wait(long tick, double timeout_s) const;
  long live_stop();            // returns the ticks served
  bool live_active() const { return live_.active; }
  // targets a session can hold; with_outputs: one with the per-tick query or pose output (a larger kernel: fewer)
  // (a shared-axes batch answers for the plain form, which is what live_start would run)
  // kernel: 0 plain, 1 with outputs, 2 the gated one (Ops::live_capacity)
  long live_capacity_targets(int kernel = 0) const {
    const Ops* o = shared_axes() ? get_ops(type_, dtype_, lanes_code_) : ops_;
    return o->live_capacity ? o->live_capacity(kernel) * o->L.tpw : 0;
  }
  // ... of the kernel the NEXT session would run (query: one with the per-tick query)
  long live_capacity_next(bool query = false) const { return live_capacity_targets(live_kernel_next(query)); }
  int live_kernel_next(bool query) const { return live_.gate.gated() ? 2 : (query || live_.pose_out) ? 1 : 0; }
  bool live_pose_output_set() const { return live_.pose_out != nullptr; }
  bool live_running() const { return live_.active && __atomic_load_n(live_.h_done + 2, __ATOMIC_ACQUIRE) == 0; }   // the relay has not left (its last store)
  // THE UPDATE POLICY OF THE BY-ID PATHS (UpdateGate, reacquire_plan.hpp; target_manager_set_update_gate).  While it is on, every
  // by-id step WITH measurements -- step_indexed, step_indexed_dev, the one-target queue (step_one / flush), step_dense_host -- is
  // gated and, with max_rejects >= 0, keeps the rejection runs and re-acquires, with the semantics of the dense calls
  // (InnovStream::gate / reacq): the indexed ones by ONE launch of the gated indexed kernel (kf_step_sep_gate_indexed_kernel; the
  // flush keeps its fused getter-table form), step_dense_host by the dense gated kernel and reacquire_kernel.  NIS and event bytes
  // come back by entry: nis -1 = no measurement on the entry, event as target_reacquire_c's table (0 without runs).  The rows the
  // kernels write live in host-mapped memory owned by the batch.  step_dense, step_sequence, step_fused and the resident mode
  // ignore the policy.  update_gate_refusal(): why this batch cannot serve a policy (no gated indexed kernel: the dense layouts,
  // several (Q, R) classes, measured-pose rows; with runs, initial covariances no longer kept), or null.
  void set_update_gate(const UpdateGate& g);   // flushes the queued one-target steps first
  const UpdateGate& update_gate() const { return pol_; }
  const char* update_gate_refusal(const UpdateGate& g) const;
  const char* update_gate_refusal() const { return update_gate_refusal(pol_); }
  // where the queued one-target steps that carry an output position (step_one, out_pos) report when they are flushed; the caller
  // clears it (nulls) before the arrays go away
  void set_gate_sink(double* nis, unsigned char* event) { sink_nis_ = nis; sink_event_ = event; }
  // One tick over the listed slots, host inputs (meas rows follow the order of `slots`).
  // nis_out / event_out [n] (or null): the policy's outputs by entry
  void step_indexed(const int* slots, long n, double dt, const double* meas_aos, const unsigned char* has, double* nis_out = nullptr,
                    unsigned char* event_out = nullptr);
  // The same with everything already on the device: idx_dev [n] = slot of entry e or a negative number (entry skipped);
  // meas_soa_dev SoA [7][ld] in the batch precision, rows in entry order.  Asynchronous.
  // nis_dev / event_dev [n] (or null: rows of the batch's own): where the policy's kernel writes, by entry -- device-visible memory
  void step_indexed_dev(const int* idx_dev, long n, double dt, const void* meas_soa_dev, long ld, const unsigned char* has_dev,
                        double* nis_dev = nullptr, unsigned char* event_dev = nullptr);
  // derived outputs of the listed entries into device arrays (row e; entries with a negative slot are left untouched)
  void outputs_indexed_dev(const int* idx_dev, long n, double* pose_dev, double* twist_dev, double* acc_dev, bool at_time, double t1);
  // One-target call of the reference's C ABI (target_manager_update / update_meas).  The step is
  // QUEUED: it runs, together with every other queued one-target step, as a single indexed launch
  // when anything reads or otherwise touches the batch (flush()).  A slot queued twice flushes first,
  // so the order of steps per target is the caller's order.
  void step_one(long slot, double dt, const double* meas7, long out_pos = -1);
  void flush();
  // One tick over every slot in slot order, host inputs (rows of meas_aos / has follow the slot order)
  void step_dense_host(double dt, const double* meas_aos, const unsigned char* has, double* nis_out = nullptr, unsigned char* event_out = nullptr);
  // The same from SoA host rows in the BATCH precision (row c of meas_soa = component c of every slot,
  // ld_host elements apart): only the rows the model reads cross PCIe (3 for the linear models, 7 for the
  // angular ones) and no conversion kernel runs.  Pinned host memory makes the copies asynchronous DMA.
  void step_dense_host_soa(double dt, const void* meas_soa, long ld_host, const unsigned char* has);

  // Derived outputs to host arrays; slots == null means all slots in order.
  void outputs(const int* slots, long n, double* pose, double* twist, double* acc, bool at_time, double t1);
  // Dense, to device arrays [size()][7] / [size()][6] / [size()][6] (doubles).
  void outputs_dev(double* pose_dev, double* twist_dev, double* acc_dev, bool at_time, double t1);
  // pose7 of every slot into row row_of_slot_dev[slot] of pose_dev (outputs_rows_kernel; rows < 0 are skipped)
  void outputs_rows_dev(double* pose_dev, const int* row_of_slot_dev);
  void outputs_one(long slot, double* pose, double* twist, double* acc, bool at_time, double t1);
  // AoS doubles [n][7] on device -> SoA [7][ld] in the batch precision on device
  void pack_meas_dev(const double* aos_dev, long n, void* soa_dev, long ld);

  // IntersectionSolver::getIntersectionTime/PoseWithSphere (src/intersection_solver.cpp:42-104)
  // for the listed slots (host arrays; slots == null: all) or, _dev, every slot to device arrays.
  // t1 is absolute; NaN means each target's own current time.
  void intersect(const int* slots, long n, double t1, const double* origin, double radius, double* delta, double* pose);
  void intersect_dev(double t1, const double* origin, double radius, double* delta_dev, double* pose_dev);

  // the same with the reference's per-solver convergence gate kept per target (intersect_gate.hpp);
  // converged [n] bytes; filt [n][2] (filtered position / angle error) optional.  `window` is the
  // reference's filters_length (intersection_solver.hpp:63, default 250); changing it resets the gates.
  void intersect_gated(const int* slots, long n, double t1, const double* origin, double radius, double pos_th,
                       double ang_th, int window, double* delta, double* pose, unsigned char* converged, double* filt);
  void intersect_gated_dev(double t1, const double* origin, double radius, double pos_th, double ang_th, int window,
                           double* delta_dev, double* pose_dev, unsigned char* converged_dev);
  // the gate alone, fed with query results that are already on the device (e.g. the outputs of the per-tick query
  // fused into the step kernels): every slot, delta [size], pose [size][7]; filt / var [size][2] optional
  void gate_update_dev(const double* delta_dev, const double* pose_dev, double pos_th, double ang_th, int window,
                       unsigned char* converged_dev, double* filt_dev, double* var_dev);

  // THE k SOONEST CROSSINGS (select_soonest.hpp; target_batch_select_soonest[_dev]) among this batch's size() entries of a query's
  // outputs already on the device: candidates are the slots with (ok == null || ok[i]) && lo <= delta[i] <= hi, ordered by
  // (delta, slot); rows count .. k-1 get the filler.  Three launches on the batch's stream, no allocation once the shard's scratch
  // is there, no host wait in the _dev form.  It reads NO record and does not go through records(): it settles no tiles, demotes
  // nothing, drops no recording and does not flush the one-target queue.  Refusals (check_soonest_args) throw before anything is
  // enqueued.  select_soonest: the same into the scratch's device result, one copy, a synchronisation; rows [k]; returns count.
  void set_soonest_scratch(SoonestScratch* s, int max_wgs) { soonest_ = s; soonest_max_wgs_ = max_wgs; }
  void select_soonest_dev(const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev, double lo, double hi, long k,
                          int* slot_out_dev, double* delta_out_dev, double* pose_out_dev, int* count_out_dev);
  long select_soonest(const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev, double lo, double hi, long k,
                      bool with_pose, SoonestRow* rows);

  // POSITION COVARIANCE AND TIME SPREAD AT A SPHERE CROSSING (crossing_cov.hpp; target_batch_crossing_cov_dev): for row i with a
  // candidate delta[i] (>= 0), Sigma = (A(tau) P A(tau)^T + Q)[0:3, 0:3] of its slot at tau = delta[i] + (t1 - its time; 0 for
  // t1 = NaN), as cov [n][6] (xx xy xz yy yz zz); with origin also sigma [n][2] = {sigma_r, sigma_t} and ok [n] =
  // sigma_r <= sigma_r_max && sigma_t <= sigma_t_max.  slots_dev == null: dense, row i is slot i, n <= size(); else a device list
  // of n <= kCrossingCovMaxRows slots (-1: none).  batch_dev (manager level): the launch serves only the rows whose entry is
  // batch_index.  Every other row of the call gets the filler (crossing_cov_fill) and costs no record word.  One launch on the
  // batch's stream, no allocation, no host wait: it may be captured.  The records are read as stored, a flagged uniform tile's
  // words from its block: no tile is settled, no shared-axes batch demoted, no recording dropped; rejection runs and the clock
  // are not touched.  The queued one-target steps run first (flush), as ahead of every reader.  Refusals
  // (check_crossing_cov_args) throw before anything is enqueued.
  void crossing_cov_dev(double t1, const double* origin, double radius, const double* delta_dev, const int* slots_dev, long n,
                        double sigma_r_max, double sigma_t_max, double* cov_dev, double* sigma_dev, unsigned char* ok_dev,
                        const int* batch_dev = nullptr, int batch_index = 0);
  // the same for a host list of slots with host arrays (staged, one synchronisation): the by-id form's building block
  void crossing_cov(const int* slots, long n, double t1, const double* origin, double radius, const double* delta, double sigma_r_max,
                    double sigma_t_max, double* cov, double* sigma, unsigned char* ok);

  // ASSOCIATION OF UNLABELLED DETECTIONS (associate.hpp; target_batch_associate[_dev]).
  //   assoc_table_dev    this batch's rows of a call's table: for every slot zhat = the position a predict-only update(dt) would
  //                      give and W = (Sigma + R[0:3, 0:3])^-1, Sigma as crossing_cov_dev forms it at tau = dt.  One launch on the
  //                      batch's stream.  The records are read as stored: no tile is settled, no shared-axes batch demoted, no
  //                      recording dropped, rejection runs and the clock are not touched; the queued one-target steps run first.
  //   associate_dev      the whole call for this batch alone (associate_batches below).
  //   associate          the host form: detections from host memory, the per-detection rows back (ids translated), one wait.
  //   grid_cell > 0      the grid form (associate_grid.hpp; target_batch_associate_grid[_dev]) with that cell edge;
  //                      0: the brute-force form.  sdiag: where the table kernel also leaves S's diagonal, [size][3] (grid form).
  void set_assoc_scratch(AssocScratch* s, int forced_chunks, long forced_buckets = 0) {
    assoc_ = s; assoc_forced_chunks_ = forced_chunks; assoc_forced_buckets_ = forced_buckets;
  }
  AssocScratch* assoc_scratch() const { return assoc_; }
  int assoc_forced_chunks() const { return assoc_forced_chunks_; }
  void assoc_table_dev(double dt, AssocRow* rows, int batch_index, double* sdiag = nullptr, bool sigma_in_w = false);   // sigma_in_w: MergeRows (track_merge_plan.hpp)
  void associate_dev(double dt, const double* det_dev, long M, double gate, long rounds, const AssocSlotOut& out, int* slot_of_det_dev,
                     double* d2_of_det_dev, int* info_dev, double grid_cell = 0.0);
  long associate(double dt, const double* det, long M, double gate, long rounds, const AssocSlotOut& out, unsigned* ids_of_det,
                 int* slot_of_det, double* d2_of_det, long* unmatched, long* n_unmatched, int* info, double grid_cell = 0.0);

  // Building blocks of the manager's all-batches sequence (TargetManager::stepSequenceAll): enqueue
  // n_ticks ticks -- each optionally followed by the own-time sphere query of every slot -- on `st`
  // without touching the batch clock, then account for them.
  struct SeqSpec {
    const void* meas_base; long tick_stride; long ld;   // tick s reads meas_base + s*tick_stride elements, SoA [7][ld]
    const unsigned char* has_base; long has_stride;     // optional masks
    double* delta_dev; double* pose_dev;                // query outputs [size] / [size][7] (overwritten every tick)
    long ring_ticks;                                    // > 0: the measurements are a ring, tick s reads entry s % ring_ticks
    PoseStream poses{};                                 // the per-tick pose stream of the batch (tick s: poses.block(s)), or none
    InnovStream innov{};                                // the per-tick innovation stream of the batch, or none
    // (a gated tick counts its accepted measurements per slot, a masked one its measured slots: on the device)
    bool all_measured() const { return meas_base && !has_base && !innov.gated(); }
    // everything a recording made from the spec refers to (recorded graphs are keyed by it)
    bool same(const SeqSpec& o) const {
      return meas_base == o.meas_base && tick_stride == o.tick_stride && ld == o.ld && has_base == o.has_base && has_stride == o.has_stride &&
             delta_dev == o.delta_dev && pose_dev == o.pose_dev && ring_ticks == o.ring_ticks && poses.same(o.poses) && innov.same(o.innov);
    }
  };
  // THE launch parameters of dense tick s of the spec (every launched dense tick is built here, once): the ring-reduced
  // measurement block and mask row, dt (a call with a time-step schedule hands every tick its own), the pose block, NIS row and
  // innovation block of tick s of the call, the gate, with query the fused own-time sphere query, with ab (and no fused query,
  // whose kernels have no A -> B form) rec_out.  No re-acquisition policy: that is enqueue_tick's, or a launch behind the
  // population tick (enqueue_after_innov_tick).  Used as it is by the manager's one-launch population tick (kf_population.hpp),
  // possible when population_ready() -- separable layout with packed groups, one (Q, R) class, no measured-pose rows to keep;
  // with ab that caller calls swap_records() once the launch is queued (and only if the returned parameters carry rec_out).
  bool population_ready() const;
  StepParams tick_params(long s, double dt, const SeqSpec& spec, bool query, const double* origin, double radius, bool ab);
  // tick s of the spec on `st`, without touching the batch clock: tick_params, the policy, the launch, the buffer swap.  With
  // query: the own-time sphere query of every slot runs inside the step kernel (one launch) where the batch has one (Q, R) class
  // and the tick no innovation stream, behind it as intersect_kernel otherwise.
  // ab: 1 = an A -> B tick (records read from the current buffer, written to the alternate one, buffers swapped; never
  // inside a stream capture: a recorded graph bakes its pointers), 0 = in place (as is every tick with an innovation stream).
  // step_sequence enqueues its ticks, eager and recorded, through here as well.
  void enqueue_tick(hipStream_t st, long s, double dt, const SeqSpec& spec, bool query, const double* origin, double radius,
                    bool reverse = false, bool ab = false);
  // What follows a population tick that carried an innovation stream (whose kernel has neither the fused query nor the pose
  // output) for this batch: the pose-writer launch into tick s's pose block and / or the own-time sphere query, as launches.
  void enqueue_after_innov_tick(hipStream_t st, long s, const SeqSpec& spec, bool query, const double* origin, double radius);
  void swap_records() { d_rec_.swap(d_rec_alt_); }
  // Building blocks of the manager's fused replay of all batches (Shard::stepFusedAll), and of step_fused_gated itself.  spec: the
  // call's measurements, masks, pose stream and innovation stream (ring_ticks, delta_dev and pose_dev unread: fused calls read
  // linearly and have no query).
  //   check_fused_call       every refusal of step_fused_gated, nothing changed (one_launch: see check_innov_stream)
  //   fused_call_one_launch  would step_fused_gated serve the call by one launch of its own
  //   fused_call_begin       touch(), demote_shared(), then the device tables of a re-acquisition policy
  //   fused_call_params      the launch parameters of the whole call (dt_tab: the schedule in device memory, or null without one)
  //   account                the clock and the measurement counter behind the call
  void check_fused_call(long n_ticks, const SeqSpec& spec, const DtSchedule& sched, bool one_launch) const;
  bool fused_call_one_launch(const SeqSpec& spec, const DtSchedule& sched) const;
  void fused_call_begin(const SeqSpec& spec);
  StepParams fused_call_params(long n_ticks, double dt, const SeqSpec& spec, const DtSchedule& sched, const double* dt_tab);
  // Behind every multi-tick call: the batch clock advances by dt x n_ticks or, with a schedule, by one te_clock_add per tick in
  // order; the measurement counter by n_ticks where all_measured (SeqSpec::all_measured).
  void account(long n_ticks, double dt, const DtSchedule& sched, bool all_measured);
  // identity of everything a recorded launch sequence refers to
  // (ops: the launch table, i.e. which kernels a recording holds -- it changes when a shared-axes batch is expanded)
  struct DevIdentity {
    const void* rec; const void* qr; const void* tbase; const void* nmbase; long n; const void* ops; const void* p0tab;
    bool same(const DevIdentity& o) const {
      return rec == o.rec && qr == o.qr && tbase == o.tbase && nmbase == o.nmbase && n == o.n && ops == o.ops && p0tab == o.p0tab;
    }
  };
  // (the tile arrays, the rejection runs and the slot -> row index are allocated and freed with the records: rec identifies them too)
  DevIdentity dev_identity() const { return DevIdentity{d_rec_.get(), d_qr_.get(), d_tbase_.get(), d_nmbase_.get(), n_, ops_, d_p0tab_.get()}; }
  void prepare() { touch(); }
  long graph_recordings() const { return graphs_.recordings(); }   // recordings made so far (what a test of the cache observes)

  // TargetInterface::getMeasuredPose (target_interface.cpp:117-121), optional: see measured_pose.hpp
  void set_keep_measurement(bool on);
  bool keep_measurement() const { return keep_meas_; }
  void measured_poses(const int* slots, long n, double* pose7_rows);   // host rows [n][7]; slots == null: all
  // KalmanFilterInterface::getQ / getR / getP0 of one target (kalman.hpp:74-89): the matrices it was created with, as
  // given (doubles, row-major).  P0 is kept on the host as a table of the distinct matrices seen (up to kP0TableMax;
  // beyond that initial_covariance() returns false).
  void class_matrices(long slot, double* Q, double* R);
  bool initial_covariance(long slot, double* P0);
  void get_state(const int* slots, long n, double* x, double* P);
  void set_state(const int* slots, long n, const double* x, const double* P, const double* unwrap);
  long long n_measurements(long slot);
  double time(long slot);
  void times(double* out);   // filter time of every slot (host array [size()])
  void synchronize();

  // bytes of HBM one predict+update cycle must move for one target (state read+write + the
  // measurement words the model reads); used by the roofline accounting
  // (with uniform tiles: of the NEXT dense tick given the tile flags, which it reads back -- it synchronises once tiles may be flagged)
  long algorithmic_bytes_per_cycle();
  long state_bytes() const { return (n_ + ops_->L.tpw - 1) / ops_->L.tpw * ops_->L.tile_bytes; }
  static long zigzag_min_bytes();   // default 128 MB (env TE_ZIGZAG_MIN_MB)
  // A -> B ticks with nontemporal stores (kf_step.hpp StepArgs::rec_out) instead of in-place read-modify-write: the policy of
  // eager dense ticks once the state is this large (default 1536 MB, env TE_PINGPONG_MIN_MB; a negative value switches it off).
  // Below it the zig-zag in place wins (the Infinity Cache still holds a useful share of the state); costs a second record buffer.
  static long pingpong_min_bytes();
  bool pingpong() const { return pingpong_min_bytes() >= 0 && state_bytes() >= pingpong_min_bytes(); }
  char* records_dev() { return records(); }

 private:
  void reserve(long n);
  void stage_reserve(long n);
  void upload_slots(const int* slots, long n);

  int type_, dtype_, lanes_code_;
  SoonestScratch* soonest_ = nullptr;   // the owning shard's (set_soonest_scratch)
  AssocScratch* assoc_ = nullptr;       // the owning shard's (set_assoc_scratch)
  int assoc_forced_chunks_ = 0;
  long assoc_forced_buckets_ = 0;       // TE_ASSOC_GRID_BUCKETS, 0 = planned (associate_grid_plan.hpp)
  int soonest_max_wgs_ = kSoonestDefaultMaxWgs;
  std::mutex* owner_lock_ = nullptr;
  const Ops* ops_;
  hipStream_t stream_;
  // DECLARATION ORDER MATTERS from here on: members are destroyed last to first, and every buffer must go before the streams
  // and events it was used on.  So the owned streams and events come first (cap_stream_; the session's inside Live, ahead of
  // its blocks), and every buffer is declared behind them.  ~Batch only ends what may still be running.
  Stream cap_stream_;
  static constexpr double kLiveStartTimeoutS = 2.0;
  struct Live {
    Event ready;
    Stream stream;                   // the resident kernel's own stream (declared ahead of the session's blocks: see above)
    bool active = false;
    bool zombie = false;            // launched, never seen running, told to stop: synchronise its stream before touching records
    PinnedBuf<char> h_block;         // host-mapped block: [0] the doorbell unless it lives behind the BAR, [64] the relay's words
    DeviceBuf<long long> bar_bell;   // the doorbell in fine-grained DEVICE memory, written by the host through the PCIe BAR (or null)
    long long* h_posted = nullptr;   // the doorbell as the host writes it (count | stop bit)
    long long* d_posted = nullptr;   // the same block as the device sees it
    int* h_done = nullptr;
    int* d_done = nullptr;
    DeviceBuf<char> d_block;         // device memory: [mirror word, padded to 64 B][progress words of the wavefronts]
    double* pose_out = nullptr;      // per-tick pose output (live_set_pose_output)
    long pose_ld = 0;
    InnovStream gate{};              // the gate of the sessions to come (live_set_gate); !gated(): none
    long waves = 0, cap_waves = 0;
    long posted = 0, max_ticks = 0;
    double dt = 0.0;
    bool all_measured = false;
    double share = 0.0;              // > 0 while the session is counted among the process's resident sessions (hip_check.hpp)
  } live_;
  std::unordered_map<std::string, int> class_index_;   // raw bytes of [Q | R] -> class
  int n_classes_ = 0, qr_cap_ = 0;
  DeviceBuf<char> d_qr_;           // [qr_cap_][N*N + K*K] in the batch precision
  DeviceBuf<int> d_cls_;           // [cap_] class of every slot
  bool flip_ = false;              // the next dense tick walks the tiles backwards (zig-zag, kf_step.hpp StepArgs::reverse)
  // Zig-zag only pays when the state does not fit the Infinity Cache.  With the plain mirror b -> n - 1 - b it cost when the
  // state is L2-resident: a tile walked backwards landed on another XCD, whose L2 does not hold it (10^5 UA fp32: 4.7 ->
  // 8.2 us per tick), hence the threshold.  The kernels now mirror the workgroups inside each class b % 8 (zigzag_map.hpp),
  // which keeps a tile on its XCD; the threshold has not been measured again with that order and stays where it was.
  bool zigzag() const { return state_bytes() >= zigzag_min_bytes(); }
  StepParams base_params();          // launches that need plain records (indexed, fused, live): behind settle_tiles()
  StepParams dense_params();         // a dense single tick: the records as stored, with the batch's tile arrays
  // The records.  records(): settled -- for everything that reads or writes P words of a record and is not a dense tick of the
  // form.  records_as_stored(): as the dense ticks leave them (the linear-covariance chunks of a flagged tile unspecified) -- for
  // the dense ticks, get_state (which honours the flags) and readers of x alone (outputs, intersections).
  char* records() { settle_tiles(); return d_rec_.get(); }
  char* records_as_stored() const { return d_rec_.get(); }
  long count_uniform(long* targets_in_them);   // flagged tiles (and the targets in them); synchronises
  bool ut_on_ = true;
  DeviceBuf<double> d_tile_blk_;   // [cap_ / tpw][L.lin_words], allocated with the records
  DeviceBuf<int> d_tile_uni_;      // [cap_ / tpw]
  bool ut_flagged_ = false;        // a promoting launch has run since the last settle: tiles may be flagged
  long dense_streak_ = 0;          // consecutive dense ticks since the last settle
  bool recording_ = false;
  void launch_step(const StepParams& p, hipStream_t st, int meas_rows = 7);   // ops_->step + the measured-pose rows when kept
  bool keep_meas_ = false;
  int host_meas_rows_ = 7;         // measurement rows the host SoA path transported for the tick being enqueued
  DeviceBuf<double> d_lastmeas_;   // [cap_][7] doubles (measured_pose.hpp), null unless keep_meas_
  std::vector<std::vector<double>> class_qr_;   // [Q | R] of every class as given (doubles)
  static constexpr size_t kP0TableMax = 4096;
  std::vector<std::vector<double>> p0_tab_;
  std::unordered_map<std::string, int> p0_index_;
  std::vector<int> slot_p0_;       // slot -> row of p0_tab_
  bool p0_kept_ = true;
  int intern_p0(const double* P0);
  DeviceBuf<char> d_rec_;          // the CURRENT records (A -> B ticks swap it with d_rec_alt_ after every launch)
  DeviceBuf<char> d_rec_alt_;      // second record buffer of the same capacity, allocated on the first A -> B tick
  char* alt_records();             // null if the device has no room for it (the batch then stays in place)
  bool alt_failed_ = false;
  DeviceBuf<TClock> d_tbase_;
  DeviceBuf<int> d_nmbase_;
  DeviceBuf<unsigned char> d_has_eff_;   // [cap_] the effective mask of a gated tick whose layout has no gated kernel (StepParams::gate_row)
  // Re-acquisition (kf_reacquire_impl.hpp): the rejection run of every slot -- library-owned, 0 at creation, follows its target
  // through erase and growth, read and written by the calls with a policy only -- and the device copies of p0_tab_ / slot_p0_.
  DeviceBuf<unsigned char> d_run_;       // [cap_], allocated with the records
  DeviceBuf<int> d_p0idx_;               // [cap_], allocated with the records; current behind prepare_reacquire()
  DirtySlots p0idx_dirty_;
  DeviceBuf<double> d_p0tab_;            // [p0tab_dev_.cap][N*N]
  P0TableMirror p0tab_dev_;
  void run_move(long src, long dst);
  DeviceBuf<unsigned char> d_miss_, d_hits_;   // [cap_] each, allocated with the records: the track counters (track_counts)
  void fill_reacquire(StepParams& p, const InnovStream& innov, long s_call) const;   // the policy's launch parameters of tick s_call of a call
  void prepare_p0_tables();              // the body of prepare_reacquire
  void prepare_fused_reacquire(const InnovStream& innov);   // ... of a fused call (whose kernel reads no table for K = 0)
  void enqueue_own_time_query(hipStream_t st, const SeqSpec& spec, const double* origin, double radius);   // intersect_kernel, every slot
  // the by-id update policy: its by-entry NIS row and event row (host-mapped, sized with the staging and queue blocks; the host
  // reads them as cached host memory, never through the write-combined BAR block)
  UpdateGate pol_{};
  PinnedBuf<char> h_pol_;                // nis double[pol_cap_] | event uchar[pol_cap_]
  char* d_pol_ = nullptr;
  long pol_cap_ = 0;
  void pol_reserve(long k);
  double* pol_nis_host() const { return reinterpret_cast<double*>(h_pol_.host()); }
  unsigned char* pol_event_host() const { return reinterpret_cast<unsigned char*>(h_pol_.host() + (size_t)pol_cap_ * sizeof(double)); }
  double* pol_nis_dev() const { return reinterpret_cast<double*>(d_pol_); }
  unsigned char* pol_event_dev() const { return reinterpret_cast<unsigned char*>(d_pol_ + (size_t)pol_cap_ * sizeof(double)); }
  // an indexed launch of k entries under the policy: rows reserved (unless the caller brings its own), tables current, p filled
  void fill_update_gate(StepParams& p, long k, double* nis_dev = nullptr, unsigned char* event_dev = nullptr);
  double* sink_nis_ = nullptr;
  unsigned char* sink_event_ = nullptr;
  long cap_ = 0;  // slots
  long n_ = 0;
  std::vector<unsigned> slot_ids_;
  TClock t_acc_{0.0, 0.0};  // batch clock: target time = t_base[slot] + t_acc_, both compensated pairs (te_clock.hpp)
  long long nm_acc_ = 0;    // batch measurement counter
  // staging for the host-array paths
  long stage_cap_ = 0;
  DeviceBuf<int> d_idx_;
  DeviceBuf<double> d_aos_;        // [stage_cap][19] doubles: inputs (p0|v0|a0, meas) and outputs
  DeviceBuf<char> d_meas_;         // SoA [7][stage_cap] in the batch precision
  DeviceBuf<unsigned char> d_mask_;
  DeviceBuf<double> d_P0_;
  long P0_cap_ = 0;
  // convergence gates (allocated on first use)
  int gate_window_ = 0;
  long gate_cap_ = 0;
  DeviceBuf<double> d_gate_ring_;
  DeviceBuf<double> d_gate_sum_;
  DeviceBuf<int> d_gate_state_;
  DeviceBuf<double> d_gate_prev_;
  void gate_reserve(int window);
  void gate_move(long src, long dst);
  void gate_reset(long first, long count);
  // Recorded sequences (step_sequence with use_graph): 64 kept, stamped on every use, so the least recently used one goes.
  // (a recording writes into the pose and innovation buffers it was recorded with, and bakes every tick's dt into its launch)
  struct SeqKey { long n_ticks; long n; char* rec; SeqSpec spec; DtKey dt; };
  SeqGraphCache<SeqKey> graphs_{64};
  void drop_graphs() { graphs_.drop(); }
  // The device table of a fused call with a time-step schedule: a fresh run of a ring per call (dt_table_ring.hpp)
  DtTableRing dttab_;
  const double* dt_table_push(const double* dt_host, long n);   // the device address of the call's n entries
  // queue of one-target creations (append with count == 1): consecutive ones with the same (t0, P0, class) become one init launch
  struct InitQueue { std::vector<unsigned> ids; std::vector<double> p0, v0, a0, P0; double t0 = 0.0; int cls = 0; long first = 0; } initq_;
  void flush_inits();
  long append_now(long first, long count, const unsigned* ids, double t0, const double* P0, bool per_target_P0, const double* p0,
                  const double* v0, const double* a0, int cls, const int* cls_of, const int* P0_index, long P0_count, bool bookkeeping,
                  const double* gather_det_dev = nullptr, const int* gather_rows_dev = nullptr);   // (gather: p0 from device rows, append_gathered)
  // queue of one-target steps (reference C ABI) and the cache that serves the one-target getters
  struct Pending { int slot; unsigned char has; double dt; double meas[7]; long out = -1; };   // out: position in the gate sink, or -1
  std::vector<Pending> pending_;
  std::vector<unsigned char> pending_mark_;
  DeviceBuf<double> d_dtper_;
  // Both live in pinned, device-mapped host memory: the kernels read the queued inputs and write the
  // outputs there directly, so a flush needs no copies; when the getter table is current and the queue holds at most
  // kFusedFlushMax targets it is ONE launch -- the step kernel writes the stepped rows and then a completion flag -- and the
  // host does not synchronise the stream but spins on that flag (wait_done; tools/launch_latency.hip: launch + flag 6.7 us
  // against 13.3 us for two launches and the runtime's wait, which is what longer queues still pay).
  void pin_reserve(long k);
  PinnedBuf<char> h_pin_;                    // idx int[cap] | dt double[cap] | meas T[7][cap] | has uchar[cap]
  char* d_pin_ = nullptr;                    // the same memory as the device sees it
  DeviceBuf<char> bar_pin_;                  // the same sections for flushes of up to one wavefront, in fine-grained device memory behind the PCIe BAR (flush)
  bool bar_pin_failed_ = false;
  long pin_cap_ = 0;
  // The getter table.  Batches up to kCacheMax build it at the first one-target getter after a change.  A larger batch
  // (up to kCacheBigMax) builds it only for a caller that really sweeps it target by target: the first kBigDirect getters
  // after a change are served one by one (a launch and a copy each), the next one builds the table; a batch that was swept
  // last time builds it at once, one that was not (a dense step followed by a single getter) goes back to single reads.
  static constexpr long kCacheMax = 16384;
  static constexpr long kCacheBigMax = 1L << 22;   // 19 doubles per target: 640 MB of pinned host memory at most
  static constexpr int kBigDirect = 64;
  long epoch_getters_ = 0;                   // one-target getters since the last change
  bool big_sweeps_ = false;                  // the last epoch of this (large) batch was a sweep
  static constexpr size_t kStateScratchKeep = 16u << 20;   // get_state's device scratch kept between calls up to this size
  DeviceBuf<char> d_state_scratch_;
  size_t state_scratch_bytes_ = 0;
  static constexpr int kCounterDirect = 4;   // single reads of a measurement counter before all of them are copied to the host
  std::vector<int> h_nm_;
  bool nm_valid_ = false;
  int nm_reads_ = 0;
  void cache_reserve(long n);
  PinnedBuf<double> h_cache_;                // [n][7] pose | [n][6] twist | [n][6] acceleration
  double* d_cache_ = nullptr;
  long cache_cap_ = 0;
  bool cache_valid_ = false;
  PinnedBuf<int> h_done_;                    // completion flag of the last flush (host-mapped), and its device alias
  int* d_done_ = nullptr;
  DeviceBuf<int> d_done_count_;              // device word: wavefronts of a multi-wavefront flush that have written their rows (StepArgs::done_count)
  static constexpr long kFusedFlushMax = 1024;   // up to this many queued targets the flush is ONE launch (flush)
  unsigned done_seq_ = 0;
  void wait_done(int seq);                   // spin on *h_done_ == seq, falling back to hipStreamSynchronize
  void touch() {                             // call before anything that changes state
    flush();
    cache_valid_ = false;
    nm_valid_ = false; nm_reads_ = 0;
    if (epoch_getters_ > 0) big_sweeps_ = epoch_getters_ > kBigDirect;   // (changes with no getter in between keep the verdict)
    epoch_getters_ = 0;
  }
  void live_release();
};

// ONE ASSOCIATION CALL over the batches of one device (associate.hpp lists the launches): the batches' table rows concatenated in
// the order given, det_dev [M][7] in device memory, out [n_batches] what each batch's slots get.  slot_of_det / batch_of_det /
// d2_of_det [M] may be null; info [4] = {matched, rounds_run, settled, 0}.  Everything on `st` (the shard's one stream), no host
// wait, no allocation unless the call is larger than every call before it on this scratch.  The arguments are the caller's to
// check (check_assoc_args); nothing is enqueued before every batch has been found to have a table kernel.
// grid_cell > 0: the grid form (associate_grid.hpp lists ITS launches; check_assoc_grid_args), info[3] = the wide slots;
// forced_buckets: TE_ASSOC_GRID_BUCKETS or 0.
void associate_batches(Batch* const* batches, int n_batches, AssocScratch& scratch, int forced_chunks, double dt, const double* det_dev, long M,
                       double gate, long rounds, const AssocSlotOut* out, int* slot_of_det, int* batch_of_det, double* d2_of_det, int* info,
                       hipStream_t st, double grid_cell = 0.0, long forced_buckets = 0);
// ... and its host form: det [M][7] in host memory is staged, the per-detection rows come back through the scratch's pinned mirror
// (one wait), slots are translated to ids (~0u: none), unmatched [M] receives the unmatched detections in ascending order.  Any
// output may be null.  Returns the matched count.
long associate_batches_host(Batch* const* batches, int n_batches, AssocScratch& scratch, int forced_chunks, double dt, const double* det, long M,
                            double gate, long rounds, const AssocSlotOut* out, unsigned* ids_of_det, int* batch_of_det, int* slot_of_det,
                            double* d2_of_det, long* unmatched, long* n_unmatched, int* info, hipStream_t st, double grid_cell = 0.0,
                            long forced_buckets = 0);

}  // namespace te
