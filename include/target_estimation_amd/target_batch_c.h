/*
 * target_batch_c.h -- batched extension of the target_manager C boundary (not in the reference).
 *
 * The reference steps one target per call under a manager-wide mutex
 * (src/target_manager.cpp:190-225).  At 10^4..10^6 targets the per-id calls cannot be the fast
 * path, so this header adds (a) array-of-ids entry points with host buffers and (b) a
 * device-resident dense path whose inputs already live in HBM (no host staging; this is what
 * bench.py times and what a multi-GPU caller uses, one manager per rank).
 *
 * Plain C ABI: pointers and sizes only.  "dev" pointers are HIP device pointers (e.g.
 * torch.Tensor.data_ptr()).  Unless stated, functions return 0 on success and a negative
 * error code (message on stderr) on failure; they never throw.
 */
#ifndef TARGET_ESTIMATION_AMD_TARGET_BATCH_C_H
#define TARGET_ESTIMATION_AMD_TARGET_BATCH_C_H

#include "target_manager_c.h"

typedef void target_batch_c; /* all targets of one (model, P layout) inside a manager */

/* model ids = the reference enum TargetManager::target_t (target_manager.hpp:38) */
#define TARGET_ANGULAR_RATES 0
#define TARGET_ANGULAR_VELOCITIES 1
#define TARGET_UNIFORM_ACCELERATION 2
#define TARGET_UNIFORM_VELOCITY 3
/* add to lanes_per_target (1, 2, 3 or 6) to store P symmetric-packed (upper triangle) in HBM */
#define TARGET_LAYOUT_SYMMETRIC_PACKED 100
/* lanes_per_target = 1 + this: store only the entries of P inside an axis group (exact when Q, R and
 * P0 do not couple different axes, as in every shipped model file; refused otherwise) */
#define TARGET_LAYOUT_AXIS_SEPARABLE 200
/* lanes_per_target = 1 + this: axis-separable with each group block stored as its upper triangle */
#define TARGET_LAYOUT_AXIS_SEPARABLE_PACKED 300
#define TARGET_DTYPE_F64 0
#define TARGET_DTYPE_F32 1

#ifdef __cplusplus
extern "C" {
#endif

/* ---- construction ---------------------------------------------------------------------- */
/* file may be NULL (no default model: use the *_typed initialisers, as the reference's
 * default-constructed TargetManager, target_manager.cpp:106-109).  dtype: TARGET_DTYPE_*.
 * lanes_per_target: 0 = automatic, checked per init call:
 *   - Q, R and P0 do not couple different axis groups: the axis-separable layout -- with each group block
 *     stored as its upper triangle (1 + TARGET_LAYOUT_AXIS_SEPARABLE_PACKED) when the matrices are also
 *     exactly symmetric, with full group blocks (1 + TARGET_LAYOUT_AXIS_SEPARABLE) otherwise;
 *   - coupled but exactly symmetric: the dense kernel on the upper triangle of P
 *     (G + TARGET_LAYOUT_SYMMETRIC_PACKED, G = lanes per target: 1 or 3 depending on the model);
 *   - anything else: the dense kernel on the full P with the tuned G of (model, dtype).
 * Explicit: 1, 2, 3 or 6 (dense, full P), G + TARGET_LAYOUT_SYMMETRIC_PACKED with G = 1, 2, 3 or 6 where
 * the model allows it (upper triangle of P only in HBM: 44 % less traffic), or one of the two separable
 * codes.  With a packed layout P is symmetric by construction, whereas the reference's (I-KC)P is
 * symmetric only to rounding; the full layouts reproduce that rounding-level asymmetry (the
 * axis-separable full-block layout is bit-identical to the dense kernel). */
target_manager_c* target_manager_new_ex(const char* file, int dtype, int lanes_per_target);
/* all launches of this manager go to `hip_stream` (a hipStream_t; NULL = default stream) */
int target_manager_set_stream(target_manager_c* self, void* hip_stream);
int target_manager_synchronize(target_manager_c* self);
/* rt_logger-equivalent snapshots (the reference publishes measurement / pose / twist / acceleration / covariance per
 * target, src/target_interface.cpp:32-40): with a directory set (here or by env TARGET_ESTIMATION_LOG_DIR) every
 * target_manager_log() appends one row per selected target to <dir>/time_<id>, meas_pose_<id>, est_pose_<id>,
 * est_twist_<id> (the files of the reference's test and plot script, test/target_manager_test.cpp:164-168,
 * matlab/plot_target_manager_test.m:9-13) and pose_<id> ([xyz rpy]), est_acc_<id>, covariance_<id> (P, row-major), in
 * the text format of the reference's writeTxtFile (utils.hpp:96-120).  Selected = target_manager_set_log_targets, or
 * every target while there are at most 64; otherwise one <channel>_all file per channel with the id in front of every
 * row.  Files stay open between calls; one buffered write per file per call.  NULL or "" switches logging off (log()
 * is then a no-op, as the reference without LOGGER_ON).  A directory switches the measured-pose rows on. */
int target_manager_set_log_directory(target_manager_c* self, const char* dir);
int target_manager_set_log_targets(target_manager_c* self, const unsigned int* ids, long n);   /* n == 0: automatic */
/* TargetInterface::getMeasuredPose (include/target_estimation/target_interface.hpp:130, src/target_interface.cpp:117-121,
 * :142-146): the last measurement of a target, [0 0 0 0 0 0 1] before the first.  The filters never read it back, so it is
 * kept only on request: one row of 7 doubles per target beside the records, written by a small kernel behind every
 * step (56 B per measured target per tick; off by default).  The getter returns false for an unknown id or when the
 * rows are not kept.  Linear models fed through target_batch_step_host (x y z only) report the identity orientation. */
int target_manager_set_keep_measurement(target_manager_c* self, int on);
bool target_manager_get_measured_pose(target_manager_c* self, unsigned int id, double* pose7);
/* TargetInterface::getPeriodEstimate (target_interface.hpp:94, src/target_interface.cpp:80-87): 2 pi / |omega| of the
 * current twist, -1 if the target is not rotating */
bool target_manager_get_period_estimate(target_manager_c* self, unsigned int id, double* period);
/* TargetInterface::getEstimatedTransform (target_interface.hpp:106, src/target_interface.cpp:95-98): the isometry T_ as
 * a row-major 4x4 matrix [R t; 0 0 0 1] */
bool target_manager_get_estimated_transform(target_manager_c* self, unsigned int id, double* T16);
/* TargetInterface::getN / getM (target_interface.hpp:142,148); 0 for an unknown id */
int target_manager_get_n(target_manager_c* self, unsigned int id);
int target_manager_get_m(target_manager_c* self, unsigned int id);
/* getTarget(id)->getEstimator()->getQ() / getR() / getP0() (include/target_estimation/kalman.hpp:74,79,89): the matrices
 * the target was created with, row-major doubles (Q, P0: n*n; R: m*m); any pointer may be NULL.  false: unknown id, or
 * (P0 only) the manager saw more than 4096 distinct P0 matrices for this model and stopped mirroring them. */
bool target_manager_get_model_matrices(target_manager_c* self, unsigned int id, double* Q, double* R, double* P0);
const char* target_manager_last_error(void);

/* TargetManager::init(type,id,dt0,t0,Q,R,P0,p0,v0,a0), target_manager.hpp:85-87.
 * Q, P0: n*n row-major; R: m*m; v0, a0 may be NULL (zeros). */
int target_manager_init_typed(target_manager_c* self, int type, unsigned int id, double dt0, double t0,
                              const double* Q, const double* R, const double* P0, const double* p0,
                              const double* v0, const double* a0);
/* n targets at once with the manager's default model; p0 [n][7], v0/a0 [n][6] or NULL.
 * Existing ids are skipped.  Returns the number created (or < 0). */
long target_manager_init_batch(target_manager_c* self, const unsigned int* ids, long n, double dt0, double t0,
                               const double* p0, const double* v0, const double* a0);
long target_manager_init_batch_typed(target_manager_c* self, int type, const unsigned int* ids, long n, double dt0,
                                     double t0, const double* Q, const double* R, const double* P0,
                                     int per_target_P0, const double* p0, const double* v0, const double* a0);
/* n targets whose model parameters come from a table of n_classes sets: Q [n_classes][ns*ns], R [n_classes][m*m],
 * P0 [n_classes][ns*ns] (row-major), class_of [n] = the row of target i.  The reference lets every target carry its own
 * Q, R, P0 (TargetManager::init, target_manager.hpp:85-87); here all classes of one layout live in ONE batch -- a (Q, R)
 * table in HBM plus a class index per target -- so a tick is still one launch per motion model, however many classes
 * there are.  (The one-set initialisers above do the same: a new (Q, R) for a model joins that model's batch as a new
 * class.)  Existing ids are skipped.  Returns the number created (or < 0). */
long target_manager_init_batch_classes(target_manager_c* self, int type, const unsigned int* ids, long n, double dt0, double t0,
                                       long n_classes, const double* Q, const double* R, const double* P0,
                                       const unsigned int* class_of, const double* p0, const double* v0, const double* a0);
/* TargetManager::erase, target_manager.cpp:227-241.  1 = erased, 0 = unknown id. */
int target_manager_erase(target_manager_c* self, unsigned int id);
/* the same for n ids in one call: one compaction launch per batch instead of one launch per target
 * (a timeout storm in the ingest stage).  Unknown or repeated ids print the reference's message and are
 * skipped.  Returns the number erased (or < 0). */
long target_manager_erase_batch(target_manager_c* self, const unsigned int* ids, long n);
long target_manager_size(target_manager_c* self);
/* TargetManager::getAvailableTargets (ascending ids), target_manager.cpp:126-133 */
long target_manager_get_available_targets(target_manager_c* self, unsigned int* ids_out, long capacity);

/* ---- array-of-ids calls, host buffers ---------------------------------------------------- */
/* for i < n: has_meas[i] ? update(ids[i], dt, meas[i]) : update(ids[i], dt); meas [n][7] may be
 * NULL (predict only), has_meas may be NULL (all measured).  An id that appears twice is stepped twice,
 * in order, as the reference's loop would.
 * Calls of node-tick size (up to 1024 ids, every batch of the manager at most 16384 targets) are queued like the
 * reference's one-target calls and run as one launch at the next read; target_manager_get_est_batch of that size
 * reads the host-resident rows that launch wrote (40 targets: 23 us per update + read-back, 400: 45 us; larger calls
 * stage their arrays and resolve ids on the device from 8192; TE_SMALL_BATCH_QUEUE).  Same results.
 * Returns the number of known ids stepped. */
long target_manager_update_meas_batch(target_manager_c* self, const unsigned int* ids, long n, double dt,
                                      const double* meas, const unsigned char* has_meas);
/* TargetManager::update(dt): predict every target, target_manager.cpp:220-225 */
int target_manager_update_all(target_manager_c* self, double dt);
/* any of pose [n][7], twist [n][6], acceleration [n][6], found [n] may be NULL */
long target_manager_get_est_batch(target_manager_c* self, const unsigned int* ids, long n, double* pose,
                                  double* twist, double* acceleration, unsigned char* found);
/* TargetInterface::getEstimatedPose(t1) / Twist(t1) / Acceleration(t1) (src/types, target_interface.cpp:123-140) */
long target_manager_get_est_at_batch(target_manager_c* self, const unsigned int* ids, long n, double t1,
                                     double* pose, double* twist, double* acceleration, unsigned char* found);
/* getTarget(id)->getEstimator()->getState()/getP() for ids of ONE model: x [n][ns], P [n][ns*ns]
 * row-major.  Returns the state size ns, or < 0. */
long target_manager_get_state_batch(target_manager_c* self, const unsigned int* ids, long n, double* x, double* P);
/* TargetInterface::getTime() */
int target_manager_get_time(target_manager_c* self, unsigned int id, double* t);

/* ---- sphere intersection (IntersectionSolver, src/intersection_solver.cpp:42-104) -------------- */
/* Time from t1 (absolute) to the first crossing of the sphere |p - origin| = radius along the
 * extrapolated trajectory p + v d + a d^2/2 (smallest real root of the quartic; -1 if none, if
 * it is negative, if the target has zero acceleration -- uniform_velocity and angular_velocities
 * targets never intersect in the reference -- or if the id is unknown).
 * Replaces IntersectionSolver::getIntersectionTimeWithSphere, intersection_solver.cpp:42-89. */
double target_manager_get_intersection_time_with_sphere(target_manager_c* self, unsigned int id, double t1,
                                                         const double* origin, double radius);
/* Pose at t1 + delta ([0 0 0 0 0 0 1] if none); returns whether an intersection exists.  Replaces
 * IntersectionSolver::getIntersectionPoseWithSphere, intersection_solver.cpp:91-104, WITHOUT its
 * moving-average convergence gate (:105-120; the gated form is target_manager_intersect_sphere_converged_batch below).
 * delta may be NULL. */
bool target_manager_get_intersection_pose_with_sphere(target_manager_c* self, unsigned int id, double t1,
                                                      const double* origin, double radius, double* pose,
                                                      double* delta);
/* the same for n ids: delta [n], pose [n][7] or NULL, found [n] or NULL */
long target_manager_intersect_sphere_batch(target_manager_c* self, const unsigned int* ids, long n, double t1,
                                           const double* origin, double radius, double* delta, double* pose,
                                           unsigned char* found);

/* The query above followed by the reference's convergence gate, kept PER TARGET (the reference keeps
 * one per IntersectionSolver object): two moving averages of window filters_length (<= 0: the reference
 * default 250, intersection_solver.hpp:63) over the distance and the quaternion angle between
 * consecutive intersection poses; converged[i] = both filtered errors <= their thresholds
 * (IntersectionSolver::getIntersectionPoseWithSphere, intersection_solver.cpp:91-124).  A query with no
 * intersection leaves the gate untouched and reports 0.  filtered_errors [n][2] may be NULL.
 * Costs 2 * filters_length doubles of HBM per target (allocated on first use). */
long target_manager_intersect_sphere_converged_batch(target_manager_c* self, const unsigned int* ids, long n, double t1,
                                                     double pos_th, double ang_th, const double* origin, double radius,
                                                     int filters_length, double* delta, double* pose,
                                                     unsigned char* converged, unsigned char* found, double* filtered_errors);

/* The reference's IntersectionSolver as an OBJECT (include/target_estimation/intersection_solver.hpp:56-126): a manager
 * handle plus ONE convergence gate -- two moving averages of window filters_length (default 250, :63) and the previous
 * intersection pose -- shared by every id queried through it, as the reference's members are (src/intersection_solver.cpp:
 * 19-40).  ..._get_time_with_sphere = getIntersectionTimeWithSphere (:73, .cpp:42-89); ..._get_pose_with_sphere =
 * getIntersectionPoseWithSphere (:86, .cpp:91-124): pose7 = the pose at t1 + delta, [0 0 0 0 0 0 1] if there is no
 * intersection; returns whether both filtered errors are within their thresholds.  The solver does not own the manager,
 * which must outlive it.  ..._last_errors: the filtered errors of the last call that found an intersection. */
typedef void target_intersection_solver_c;
target_intersection_solver_c* target_intersection_solver_new(target_manager_c* manager, unsigned int filters_length);
void target_intersection_solver_delete(target_intersection_solver_c* solver);
double target_intersection_solver_get_time_with_sphere(target_intersection_solver_c* solver, unsigned int id, double t1,
                                                        const double* origin, double radius);
bool target_intersection_solver_get_pose_with_sphere(target_intersection_solver_c* solver, unsigned int id, double t1, double pos_th,
                                                     double ang_th, const double* origin, double radius, double* pose7);
void target_intersection_solver_last_errors(target_intersection_solver_c* solver, double* pos_error_filtered, double* ang_error_filtered);

/* ---- device-resident dense path ---------------------------------------------------------- */
int target_manager_num_batches(target_manager_c* self);
target_batch_c* target_manager_get_batch(target_manager_c* self, int index);
target_batch_c* target_manager_get_batch_of_type(target_manager_c* self, int type);
long target_batch_size(target_batch_c* b);
int target_batch_type(target_batch_c* b);
int target_batch_dtype(target_batch_c* b);
int target_batch_state_dim(target_batch_c* b);
int target_batch_meas_dim(target_batch_c* b);
int target_batch_lanes_per_target(target_batch_c* b);
int target_batch_is_symmetric_packed(target_batch_c* b);
/* 0 full P, 1 symmetric-packed, 2 axis-separable, 3 axis-separable with symmetric-packed groups */
int target_batch_layout(target_batch_c* b);
/* 1 if the batch is in the SHARED-AXES storage form of layout 3, else 0.  In every shipped model file the x, y and z chains
 * have the same Q block, R entry and P0 block (and so have roll, pitch and yaw of angular_rates); the covariance recursion of a
 * [p v (a)] chain reads nothing else but dt and the target's own has-measurement bit, so inside one target those blocks are the
 * same bits on every tick.  An fp64 batch whose matrices pass that test exactly (doubles compared entry by entry, every P0
 * handed in included) stores and steps ONE block per kind of axis: same results bit for bit, fewer bytes per tick
 * (target_batch_algorithmic_bytes, target_batch_record_words and target_batch_resident_bytes_per_target report the form's
 * own figures; target_batch_layout and target_batch_lanes_per_target do not change).  The batch is expanded to the plain
 * records, once and for good, by the first call the form does not serve: a second (Q, R) class, a P0 whose blocks differ,
 * target_batch_step_fused[_poses], target_batch_live_start / target_manager_live_start_all.  TE_SHARED_AXES=0 in the environment, or
 * target_manager_set_shared_axes(m, 0) before the manager's first target is created (an error afterwards), keeps every
 * batch plain. */
int target_batch_shared_axes(target_batch_c* b);
int target_manager_set_shared_axes(target_manager_c* self, int on);
/* UNIFORM TILES, a property of batches in the shared-axes form (uniform_velocity, uniform_acceleration, angular_rates; the
 * angular_velocities kernels are built without it).  The same argument holds BETWEEN targets: two targets whose linear-chain
 * covariance words are the same bits, and which receive the same dt and the same has-measurement bit, hold the same bits after
 * the tick.  A population created in bulk and measured every tick is in that state tile after tile (a tile = the 64 targets of
 * one wavefront).  The dense step kernels find such tiles themselves -- a tile counts as uniform only after the kernel has
 * compared the bits of its lanes, and stops being one, in the same kernel, on the tick whose has-bits split it -- and keep ONE
 * copy of those words per tile (12 / 6 / 3 words: angular_rates / uniform_acceleration / uniform_velocity; about 1.5 B per
 * target of side arrays, not counted in target_batch_resident_bytes_per_target).  A uniform tile's dense tick neither reads nor
 * writes the 16-byte record chunks that hold only such words (6 / 3 / 1 of them): same results bit for bit, fewer bytes.
 * Nothing is deferred: records, blocks and flags are the complete state after every tick.  Everything that is not a dense tick --
 * by-id updates, creations, erasures, leaving the shared form -- first writes the blocks back into the
 * records (one dense pass, exact) and clears the flags; target_batch_get_state and the pose / twist / intersection getters do
 * not.  Tiles are looked at for promotion only after 2 consecutive dense ticks without such a call (TE_UNIFORM_TILES_AFTER
 * overrides), so a caller who interleaves by-id updates with dense ticks never pays that pass per tick; recorded sequences
 * always look.  TE_UNIFORM_TILES=0, or target_manager_set_uniform_tiles(m, 0) before the manager's first target (an error
 * afterwards), switches it off.
 * target_batch_uniform_tiles: the number of tiles flagged now.  It reads the flags back on the batch's stream: a SYNCHRONISING
 * call that first runs the queued one-target steps (they settle the tiles).  target_batch_algorithmic_bytes reports what the next dense tick moves given the flags (the same read-back, after the same
 * queued steps): per target of a flagged tile 32 B less per skipped chunk, plus the tile's 2 x 8 x words + 4 B of block
 * and flag traffic divided by its targets; the mean over the batch, rounded down; with no tile flagged, the form's constant. */
long target_batch_uniform_tiles(target_batch_c* b);
int target_manager_set_uniform_tiles(target_manager_c* self, int on);
/* words of one target's record in HBM: x + unwrap memory + the stored words of P */
int target_batch_record_words(target_batch_c* b);
/* number of distinct (Q, R) parameter classes among the batch's targets */
int target_batch_num_classes(target_batch_c* b);
/* bytes one predict+update cycle of one target must move ((2n + 2n^2 + 7 (+6)) * w, or
 * (2n + n(n+1) + 7 (+6)) * w for a symmetric-packed batch, (2n + 2 sum(group^2) + 7 (+6)) * w for an
 * axis-separable one) */
long target_batch_algorithmic_bytes(target_batch_c* b);
/* HBM bytes actually allocated per target (record incl. tile padding) */
double target_batch_resident_bytes_per_target(target_batch_c* b);
/* slot -> id of the dense order (slot i is row i of every dense array) */
long target_batch_slot_ids(target_batch_c* b, unsigned int* ids_out, long capacity);
/* One predict(+update) tick over every target of the batch, asynchronous on the manager's stream.
 *   meas_dev    : SoA [7][ld] in the batch precision (row c = component c of [x y z qx qy qz qw]
 *                 for all slots), or NULL for predict-only.  Linear models read rows 0..2 only.
 *   has_meas_dev: per-slot bytes, or NULL (every slot has a measurement). */
int target_batch_step(target_batch_c* b, double dt, const void* meas_dev, long ld, const unsigned char* has_meas_dev);
/* One tick of every slot from HOST measurements in SoA form and in the batch precision: row c of meas_soa_host
 * (ld_host elements per row) = component c of [x y z qx qy qz qw] for slots 0..size-1.  Only the rows the model
 * reads are copied (3 for the linear models, 7 for the angular ones): 12-24 B per target over PCIe instead of the
 * 56 B of target_manager_update_meas_batch's double[n][7], and no conversion kernel.  has_meas_host [size] or
 * NULL.  Returns after the step has been enqueued and the host arrays have been consumed. */
int target_batch_step_host(target_batch_c* b, double dt, const void* meas_soa_host, long ld_host, const unsigned char* has_meas_host);
/* n_ticks consecutive ticks = n_ticks launches of the step kernel, enqueued in one call: tick s
 * reads meas_dev + s * tick_stride elements (and has_meas_dev + s * has_stride bytes).  With
 * use_graph != 0 the launches are recorded once into a hipGraph (keyed by the arguments) and
 * replayed: for replaying recorded streams at small batch sizes, where the tick is launch-bound.
 * use_graph == 2 records the graph and launches nothing (set-up before a timed region). */
int target_batch_step_sequence(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                               const unsigned char* has_meas_dev, long has_stride, int use_graph);
/* The same with the measurements (and masks) held as a RING of ring_ticks ticks: tick s reads ring entry
 * s % ring_ticks, so one recorded graph may hold several passes over the ring (fewer graph launches). */
int target_batch_step_sequence_ring(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                                    const unsigned char* has_meas_dev, long has_stride, long ring_ticks, int use_graph);
/* The same n_ticks ticks in ONE launch: each target's state stays in registers across the ticks and
 * only the measurements are read per tick (temporal fusion; identical results).  For replaying
 * recorded streams; its throughput is an "effective" figure, not comparable with one launch per tick.
 * Batches that have no fused kernel -- several (Q, R) classes in the batch, or one of the few (model, precision, layout)
 * combinations whose fused form would spill -- are served tick by tick inside the call: same results, one launch per tick. */
int target_batch_step_fused(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                            const unsigned char* has_meas_dev, long has_stride);
/* RESIDENT ("live") mode for small batches -- a live stream without a dispatch per tick.  A 10^4-target tick is shorter than
 * the 1.5-2 us a dependent kernel launch costs, so at BASELINE.json configs[1] / configs[2] the per-tick launch IS the tick.
 * Here ONE launch stays on the device with the batch's state in registers and serves tick after tick as the host posts them:
 *   ..._live_start   launch.  meas_ring_dev / has_ring_dev: a ring of ring_ticks ticks in device memory, laid out as for
 *                    target_batch_step_sequence; tick k of the session reads entry (first_entry + k) % ring_ticks, which must
 *                    hold tick k's measurements BEFORE tick k is posted (written by a copy on another stream, or in advance;
 *                    the kernel reads them past the caches).  max_ticks bounds the session; idle_limit_s (<= 0: 10 s) is how
 *                    long a wavefront waits without news before it gives up by itself.
 *   ..._live_post    n more ticks are in the ring: one store to the doorbell word the resident kernel polls -- in device memory,
 *                    written through the PCIe BAR, where the system has a large BAR (the GPU then polls a local word instead of
 *                    reading host memory over PCIe every round: a paced tick of 10^5 targets 8.0 -> 6.6 us from C++), in host-mapped
 *                    memory otherwise or with TE_LIVE_DOORBELL=host.  Returns at once.
 *   ..._live_done    ticks that EVERY wavefront has finished;  ..._live_wait: spin until that reaches `tick` (0) or timeout (1)
 *   ..._live_stop    finish the posted ticks, write the records back, end the launch; returns the ticks served
 * Results equal those of single ticks bit for bit.  While a session is open the records in HBM are stale: any other call on
 * the batch (steps, getters, erase, init) ends the session first.  Needs the automatic layout of the shipped models
 * (axis-separable, packed groups), one (Q, R) class and a batch small enough to be fully resident: ..._live_capacity targets
 * (on an MI355X: 3.1 * 10^5 targets for the linear models, 1.8 to 2.5 * 10^5 for the angular ones in either precision -- the fp64
 * angular kernels park part of the record in LDS; a session with the per-tick query or pose output runs a larger kernel: 1.1 to 3.1 * 10^5;
 * profiles/r04_live_capacity.txt).  ..._live_start returns once the resident kernel
 * is known to run (its last workgroup says so) and fails after 2 s otherwise; the kernel runs on a high-priority stream of the
 * library's own, so that no stream of the caller shares its hardware queue (work queued behind an endless kernel waits for its end).  Posting faster than the device serves is fine: a wavefront that is behind catches up
 * without polling.
 * Sessions of one PROCESS share the device: the library counts the resident sessions of the process (all managers) and refuses a
 * start whose wavefronts do not fit next to the ones already resident ("do not fit the device together") instead of launching a
 * grid that can only start in part.  A session of ANOTHER process is not seen: there the 2 s start check is what reports it.
 * While any session of the process is resident, calls that would FREE device memory (a batch that grows, measured-pose rows
 * switched off, large get_state requests, a destroyed manager) do not call hipFree -- it synchronises the device and would block
 * until that session ends -- but put the memory on a list that is freed when the last session has left. */
int target_batch_live_start(target_batch_c* b, double dt, const void* meas_ring_dev, long tick_stride, long ld,
                            const unsigned char* has_ring_dev, long has_stride, long ring_ticks, long first_entry, long max_ticks,
                            double idle_limit_s);
/* Per-tick pose output of the sessions started AFTER this call (also through target_manager_live_start_all): pose_soa_dev =
 * device memory, SoA [7][ld] doubles (row c = component c of [x y z qx qy qz qw] for slots 0..size-1), NULL = off.  The resident
 * kernel writes the estimated pose of every target after every tick -- what the reference's node publishes every tick
 * (src/target_manager_ros.cpp:78-87) -- through the caches and before the tick counts as done: copy the buffer on another stream
 * after ..._live_done reached tick k and it holds the poses of a tick >= k (exactly k when one tick is posted at a time). */
int target_batch_live_set_pose_output(target_batch_c* b, double* pose_soa_dev, long ld);
/* THE GATE INSIDE A RESIDENT SESSION.  Sticky like ..._live_set_pose_output: the sessions started AFTER this call (also through
 * target_manager_live_start_all, for each batch it was set on) decide the NIS validation gate between prediction and update,
 * keep the rejection runs and re-initialise a lost target INSIDE the resident kernel, tick after tick -- no launch per tick.
 *   nis_max == 0 or nis == NULL   the gate is off: sessions are exactly the plain ones.
 *   nis_max > 0 (+inf included)   the session is gated.  nis->nis_dev is required (it reports the decisions, as in the launched
 *                                 calls; a stride of 0 keeps it to one row); nis->innov_dev must be NULL.
 *   reacq (or NULL: gate only)    the policy of target_batch_step_sequence_reacquire: max_rejects 0..127, event rows or none.
 * Per slot and tick the semantics are those of target_batch_step_sequence_gated / ..._reacquire, word for word: the decision is
 * (double)NIS <= nis_max (a NaN rejects); an accepted slot leaves in the bits of the ungated tick with mask 1, a rejected one in
 * those of the ungated tick with mask 0 (state, covariance, unwrap memory, measurement counter); NIS is reported either way, -1
 * without a measurement; the rejection run follows target_reacquire_c's table, and a re-initialised slot becomes bit for bit
 * what a fresh target created from this tick's measurement gets (v0 = a0 = 0, the slot's own P0, unwrap memory 0, clock and
 * counter untouched; the finiteness rule unchanged).  The per-tick pose output and the per-tick query of the same session see
 * the re-initialised state.
 * ROWS.  Tick k of the session, counted from 0 at ..._live_start, writes NIS row b = (ring_ticks > 0 ? k % ring_ticks : k) at
 * nis_dev + b * nis_tick_stride, and its event row likewise through reacq's ring_ticks / tick_stride.  Columns >= size are never
 * written.  With ring_ticks == 0 and a non-zero stride the caller provides max_ticks rows.  Both rows leave the kernel as the
 * pose output does -- written through the caches, before the tick counts as done -- so a consumer may copy them on another
 * stream once ..._live_done has reached k + 1, without ending the session.
 * RUNS.  The session reads every slot's rejection run (the byte the dense calls use) at its start, keeps it in a register and
 * writes it back with the records when the kernel leaves -- at ..._live_stop, or by itself after the idle limit.  "Any other call
 * on the batch ends the session first" covers target_batch_rejection_runs and target_manager_get_rejection_run as well.
 * REFUSED (negative return, target_manager_last_error, nothing launched or changed): nis_max < 0 or NaN; a gate without nis_dev;
 * innov_dev != NULL; ld < size; a stride in (0, ld) or negative; ring_ticks < 0; max_rejects outside 0..127; a policy without a
 * gate; a batch that keeps measured poses; max_rejects > 0 on a batch that no longer keeps its initial covariances; a batch
 * without resident kernels or with several (Q, R) classes.  A batch that grew past ld since the call is refused at ..._live_start.
 * The gated session runs a kernel of its own (the pose / query session's tick loop with the gate inside; a plain and a pose /
 * query session keep theirs): once a gate is set, ..._live_capacity reports THAT kernel's capacity, at most the ungated figure.
 * ..._live_gate_served: 1 if this batch has a gated resident kernel, 0 if not (..._live_set_gate then refuses), -1 on error.  Every
 * (model, precision) with resident kernels has one, at zero scratch (profiles/live_gate_kernel_resources.txt).
 * Not served: the innovations nu (NIS only, as by id).  (A launched fused call gates and re-acquires through
 * target_batch_step_fused_gated below.) */
struct target_innov_stream_c;   /* (both defined below, with the launched calls they were made for) */
struct target_reacquire_c;
int target_batch_live_set_gate(target_batch_c* b, double nis_max, const struct target_innov_stream_c* nis, const struct target_reacquire_c* reacq);
int target_batch_live_gate_served(target_batch_c* b);
int target_batch_live_post(target_batch_c* b, long n_ticks);
/* n_ticks doorbells of ONE tick each, back to back (what a caller's loop of ..._live_post(b, 1) does, without its call overhead) */
int target_batch_live_post_each(target_batch_c* b, long n_ticks);
long target_batch_live_done(target_batch_c* b);
int target_batch_live_wait(target_batch_c* b, long tick, double timeout_s);
long target_batch_live_stop(target_batch_c* b);
long target_batch_live_capacity(target_batch_c* b);
/* 1 while the session's resident kernel is there (serving or waiting), 0 once it has left -- after ..._live_stop, or by itself after
 * idle_limit_s without news (the records are back in HBM then; ..._live_stop still has to be called to close the session) */
int target_batch_live_running(target_batch_c* b);
/* n_ticks ticks of EVERY batch of the manager in one call (BASELINE.json configs[3]/[4]: several motion
 * models per GPU, optionally with the per-tick sphere query "fused on-GPU").  per_batch[i] describes
 * batch i (target_manager_get_batch order): measurements as for target_batch_step_sequence, plus the
 * device outputs of the query (delta [size], pose [size][7] or NULL; overwritten every tick) when
 * query != 0.  The query is the own-time one (t1 = each target's current time).  Batches are
 * independent.  When every non-empty batch is a one-class batch in the axis-separable layout with packed
 * groups (the automatic choice for the shipped model files) and there are at least two, a tick of ALL of
 * them is ONE launch (csrc/kf_step_sep.hpp kf_step_population_kernel; target_manager_population_tick says
 * whether that holds): nothing then depends on which hardware queues the runtime gives to concurrent
 * streams.  Otherwise there is a launch per batch per tick; with use_graph != 0 the batches' chains are
 * recorded as parallel branches of ONE hipGraph (use_graph == 2: record only).  Results are identical to
 * calling target_batch_step (+ target_batch_intersect_sphere_dev with a NaN t1) per batch per tick. */
typedef struct target_batch_sequence_c {
  const void* meas_dev; long tick_stride; long ld;
  const unsigned char* has_meas_dev; long has_stride;
  double* delta_dev; double* pose_dev;
  long ring_ticks;   /* > 0: meas_dev / has_meas_dev hold a ring of that many ticks, tick s reads entry s % ring_ticks; 0: linear */
} target_batch_sequence_c;
int target_manager_step_sequence_all(target_manager_c* m, long n_ticks, double dt, const target_batch_sequence_c* per_batch,
                                     long n_batches, int query, const double* origin, double radius, int use_graph);
/* 1 if target_manager_step_sequence_all currently steps all batches with one launch per tick, 0 if with a launch per
 * batch, -1 on error (semantics served: every target of every model each tick, src/target_manager.cpp:190-225) */
int target_manager_population_tick(target_manager_c* m);
/* Per-tick poses from launched ticks.  The reference's node steps every target and then publishes every target's pose, every
 * tick (src/target_manager.cpp:190-225, src/target_manager_ros.cpp:78-87).  The ..._poses forms of the launched calls below do
 * both: after tick s of the call the estimated pose of every target at its own time -- getEstimatedPose(), the value
 * target_batch_get_est_dev returns, bit for bit -- is in the caller's device buffer:
 *   pose_dev + b * tick_stride,  b = (ring_ticks > 0 ? s % ring_ticks : s),  doubles SoA [7][ld]: row c = component c of
 *   [x y z qx qy qz qw], column j = slot j (target_batch_slot_ids order; columns >= the batch size are never written).
 * tick_stride 0: every tick overwrites the one block.  Poses are written for EVERY target on every tick, masked and predict-only
 * ticks included.  fp32 batches derive the pose in fp32 and store it as double, as target_batch_get_est_dev does.
 * Who writes them: the kernel that did the step, from the posterior still in registers, for the axis-separable layouts of
 * one-class batches (the automatic layout of the shipped models) -- single ticks, temporally fused ticks, the fused query, A -> B
 * ticks, and the one-launch population tick: one launch per tick, as without poses.  TWO launches per tick (the step as without
 * poses, then a pose-writer launch that reads the records back) for: the dense layouts (coupled Q / R / P0, or an explicit
 * lanes_per_target outside 201 / 301), batches with several (Q, R) classes, and a target_batch_step_fused_poses of those
 * layouts (served tick by tick).  target_batch_step_fused_poses is one launch for the whole call except on fp32 angular_rates and
 * uniform_acceleration batches with packed groups (the automatic fp32 layout of those models), whose temporally fused POSE kernels
 * would spill: those are served tick by tick, one POSE launch per tick (profiles/r05_pose_kernel_resources.txt).
 * A NULL `poses` (or per_batch_poses), or a NULL pose_dev, gives the existing call: same results, same kernels.  Bad arguments
 * (ld < batch size, tick_stride in (0, 7 * ld) or negative, ring_ticks < 0) return a negative code with target_manager_last_error
 * set, and nothing is launched.  The measurements, masks, rings, use_graph (0 / 1 / 2: a recorded graph is keyed by the pose
 * stream too), the fused query and the return codes are those of target_batch_step_sequence[_ring], target_batch_step_fused and
 * target_manager_step_sequence_all; ring_ticks of ..._step_sequence_poses is the measurement ring (0: linear). */
typedef struct target_pose_stream_c {
  double* pose_dev;   /* device memory; NULL = no poses for this batch */
  long ld;            /* >= batch size */
  long tick_stride;   /* doubles between the blocks of consecutive ticks (>= 7 * ld); 0 = every tick overwrites one block */
  long ring_ticks;    /* > 0: tick s writes block s % ring_ticks; 0: block s */
} target_pose_stream_c;
int target_batch_step_sequence_poses(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                     long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                     const target_pose_stream_c* poses, int use_graph);
int target_batch_step_fused_poses(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                                  const unsigned char* has_meas_dev, long has_stride, const target_pose_stream_c* poses);
/* per_batch_poses[i]: the pose stream of batch i (NULL: none for any batch) */
int target_manager_step_sequence_all_poses(target_manager_c* m, long n_ticks, double dt,
                                           const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                           long n_batches, int query, const double* origin, double radius, int use_graph);
/* Per-tick innovations and NIS from launched ticks.  The two numbers that say how well the filter and the measurements agree
 * exist inside every update -- the innovation nu = y - x^-[0:m] and the inverse innovation covariance S^-1
 * (src/kalman.cpp:92-93, :137-138) -- and the ..._innov forms of the launched calls below stream them out: after tick s of the
 * call, with b = (ring_ticks > 0 ? s % ring_ticks : s) and column j = slot j (target_batch_slot_ids order; columns >= the batch
 * size are never written),
 *   nis_dev[b * nis_tick_stride + j]                        = nu^T S^-1 nu of that tick, the normalised innovation squared;
 *   innov_dev + b * innov_tick_stride, doubles SoA [m][ld]  : row c = nu_c, c = 0 .. m - 1 (only if innov_dev is not NULL).
 * m is 3 for the linear models (x y z) and 6 for the angular ones (x y z roll pitch yaw).  The angular components are taken
 * against the UNWRAPPED measured rpy, i.e. the same y the update uses; S^-1 is the inverse the gain uses, not a second one.
 * fp32 batches compute in fp32 and store as double.  A stride of 0 overwrites one row / block every tick.
 * A target without a measurement on that tick (mask 0, or a predict-only tick: meas_dev NULL) gets NIS = -1 and nu = 0.
 * `poses` / `per_batch_poses` and the fused `query` keep their meaning and their results, bit for bit; so does the state.
 * Who writes it: the kernel that did the step, while the values are in registers, for one-class batches in the axis-separable
 * layouts (lanes 201 and 301, and 301 in the shared-axes storage form with or without uniform tiles -- the form serves the stream
 * and the batch stays in it): single dense ticks and the one-launch population tick, one launch per tick as without the stream.
 * A tick with an innovation stream runs IN PLACE: the A -> B variant is not taken for that call (same bits).  With `poses` in the
 * same call the step is followed by the pose-writer launch, with query != 0 by the query launch per batch (what
 * target_batch_intersect_sphere_dev runs): those combinations have no kernel of their own.  The dense layouts (coupled
 * Q / R / P0, an explicit lanes_per_target outside 201 / 301, the symmetric-packed EKF) and batches with several (Q, R) classes
 * are served by one innovation-writer launch BEFORE each tick's step -- it reads the records, the class rows and the unwrap
 * memory and writes nothing else -- and then step as without the stream.
 * use_graph 0 / 1 / 2 as for ..._poses: a recorded graph is keyed by the innovation stream too.  Bad arguments (ld < batch size,
 * nis_tick_stride in (0, ld), innov_tick_stride in (0, m * ld), a negative value, ring_ticks < 0) return a negative code with
 * target_manager_last_error set, and nothing is launched.  A NULL `innov` (or per_batch_innov), or a NULL nis_dev, gives exactly
 * the ..._poses call.  target_batch_algorithmic_bytes keeps reporting the plain tick: the stream adds 8 B per target and tick
 * for NIS, plus 8 * m B for the innovations.
 * target_batch_step_fused has its innovation stream in target_batch_step_fused_gated below (nis_max 0).
 * Not served: the resident mode (target_batch_live_*) reports NIS rows only,
 * through the gate of its sessions (target_batch_live_set_gate), not nu; by id only NIS is
 * reported (target_manager_update_meas_batch_gated below), not nu. */
typedef struct target_innov_stream_c {
  double* nis_dev;          /* device memory; NULL = no innovation stream for this batch */
  double* innov_dev;        /* device memory or NULL: NIS only */
  long ld;                  /* >= batch size */
  long nis_tick_stride;     /* doubles between the NIS rows of consecutive ticks (>= ld); 0 = every tick overwrites one row */
  long innov_tick_stride;   /* the same for the [m][ld] innovation blocks (>= m * ld); 0 = overwrite */
  long ring_ticks;          /* > 0: tick s writes block s % ring_ticks; 0: block s */
} target_innov_stream_c;
int target_batch_step_sequence_innov(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                     long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                     const target_pose_stream_c* poses, const target_innov_stream_c* innov, int use_graph);
/* per_batch_innov[i]: the innovation stream of batch i (NULL: none for any batch) */
int target_manager_step_sequence_all_innov(target_manager_c* m, long n_ticks, double dt,
                                           const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                           const target_innov_stream_c* per_batch_innov, long n_batches,
                                           int query, const double* origin, double radius, int use_graph);
/* ---- The NIS validation gate inside launched ticks.
 * A chi-square gate around the Kalman update, decided INSIDE the tick, between prediction and update: the ..._innov calls with a
 * threshold nis_max on NIS = nu^T S^-1 nu.  A launched dense tick with a gate treats a target as follows.
 *   no measurement on the tick (mask 0): as without a gate -- predict only, NIS -1, zero innovations;
 *   measurement present: x^-, P^-, the unwrapped angles, nu and S^-1 are formed as the update forms them and NIS is summed in the
 *     ..._innov order (chains axis-ascending, the EKF attitude group last).  The measurement is ACCEPTED iff (double)NIS <= nis_max
 *     evaluates true -- a NaN NIS (a NaN anywhere in the measurement) rejects; fp32 batches sum NIS in fp32 and compare the double
 *     that the stream stores.  The NIS row and the innovation block report NIS and nu of the measurement whether or not it was
 *     accepted: a consumer recovers the decision exactly as 0 <= nis <= nis_max;
 *   accepted: the update -- bit for bit the ungated tick with mask 1;
 *   rejected: bit for bit the ungated tick with mask 0 (the reference's update(dt)): state, covariance, the unwrap memory (not
 *     advanced) and the target's measurement counter (not incremented) are those of a predict-only tick, and no NaN of the
 *     rejected measurement reaches the record.
 * So a gated call leaves every target in the bits the ungated call leaves with the mask has & (0 <= nis <= nis_max), nis read from
 * the gated call's own stream.  chi-square 0.99 quantiles for the user's convenience: 11.345 for m = 3 (the uniform models),
 * 16.812 for m = 6 (the angular models).
 * nis_max == 0 (or a NULL per_batch_nis_max): no gate for that batch, exactly the ..._innov call.  nis_max > 0, +inf included:
 * gated.  nis_max < 0 or NaN, or nis_max > 0 with a NULL `innov` / nis_dev (the NIS row reports the decisions; a stride of 0 keeps
 * it to one line): a negative return code, target_manager_last_error set, nothing launched.
 * One-class batches in the axis-separable layouts decide inside the step kernel (and inside the population kernel where the
 * manager's tick is one launch); every other layout's innovation-writer launch is followed by a small launch that forms the effective
 * mask from the NIS row just written, into a row the library owns, and the plain step takes that row -- three launches per tick,
 * one more than ..._innov.  Poses and the fused query in the same
 * call, use_graph (a recorded graph is keyed by the gate too) and every other argument: as for ..._innov.
 * A temporally fused call gates through target_batch_step_fused_gated below.  The resident mode gates inside its sessions (target_batch_live_set_gate).  The by-id / indexed launches, the one-target symbols and the Eigen
 * facade are gated through the sticky policy of target_manager_set_update_gate below. */
int target_batch_step_sequence_gated(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                     long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                     const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max, int use_graph);
/* per_batch_nis_max[i]: the gate of batch i (NULL: none for any batch) */
int target_manager_step_sequence_all_gated(target_manager_c* m, long n_ticks, double dt,
                                           const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                           const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max, long n_batches,
                                           int query, const double* origin, double radius, int use_graph);
/* ---- Re-acquisition of lost tracks inside the gated ticks.
 * A bare validation gate locks out: a target whose measurements move off its prediction for good is rejected on every tick from
 * then on.  The ..._reacquire calls are the ..._gated calls with a policy K = max_rejects on consecutive rejections, kept and
 * acted on inside the launched ticks.
 * Every slot has a REJECTION RUN c: one unsigned byte the library owns, 0 at creation.  It follows its target through erase
 * compaction and capacity growth.  Only the calls of this section read or write it; every other call, the plain ..._gated ones
 * included, leaves it alone.  A gated tick run through these calls with a policy treats a slot as follows.
 *   no measurement on the tick (mask 0, or a predict-only tick)   c unchanged                          event byte 0
 *   measured and accepted (0 <= nis <= nis_max, nis being the
 *     double the stream stores -- the step's own decision)         c = 0                                event byte 0
 *   measured and rejected, not re-initialised                     c' = min(c + 1, 127), stored c = c'  event byte c'
 *   measured and rejected, re-initialised                         c' = min(c + 1, 127), stored c = 0   event byte 0x80 | c'
 * A rejected slot is RE-INITIALISED iff K > 0 and c' >= K and the initial state formed from this tick's measurement is finite in
 * every component -- for the angular models after the quaternion has become roll, pitch, yaw, so a NaN measurement or a zero
 * quaternion never re-initialises.
 * Re-initialisation: behind the tick's step the slot's record becomes, bit for bit, what the creation of a fresh target writes
 * with p0 = this tick's measurement in the batch precision as the tick read it, v0 = a0 = 0, P0 = the slot's own initial
 * covariance (the P0 that target_manager_get_model_matrices returns for it) and unwrap memory 0.  The target keeps its slot, its id,
 * its class, its clock (advanced by dt like every other slot) and its measurement counter: the rejected tick did not increment
 * it and the re-initialisation does not touch it.  State, covariance, unwrap memory and counters of every slot that is not
 * re-initialised are those of the ..._gated call, bit for bit; K = 0 counts only.  Poses and the query in the same call see the
 * re-initialised state.  The convergence gates' moving averages of a re-initialised target are not reset.
 * event_dev (or NULL): after tick s, row b = (ring_ticks > 0 ? s % ring_ticks : s) at event_dev + b * tick_stride holds the event
 * byte of every slot (column = slot); columns >= batch size are not written.
 * Refused with a negative code, target_manager_last_error set and nothing launched: a policy without a gate (nis_max == 0);
 * max_rejects outside 0..127; event rows with ld < batch size, tick_stride in (0, ld), a negative tick_stride or ring_ticks; a batch
 * that keeps measured poses (target_manager_set_keep_measurement); a batch that no longer keeps its initial covariances (more than
 * 4096 distinct ones); everything ..._gated refuses.  A NULL policy (or NULL per_batch_reacq) is exactly the ..._gated call.
 * How: one small launch per batch behind each measured tick's step (behind the population launch where the manager's tick is
 * one launch) and ahead of that tick's pose-writer and query launches, recorded with the tick; a recorded graph is keyed by the
 * policy too.  It streams about 11 B per target and tick (NIS, mask byte, run, event) and touches records only in wavefronts
 * that re-initialise.  A tile of a shared-axes batch that is re-initialised while flagged uniform is settled first; the batch
 * stays in the form.
 * A gate at a chi-square quantile re-initialises often on a stream that is not chi-square consistent:
 * choose nis_max for the outliers to be kept out, K for the time a lost target may coast.
 * A temporally fused call keeps the runs and re-acquires through target_batch_step_fused_gated below, the resident mode inside
 * its sessions (target_batch_live_set_gate).  Not served: M-of-N logic other than K consecutive; a velocity from two
 * measurements.  The by-id / indexed launches, the one-target symbols and the Eigen facade re-acquire through the sticky policy
 * of target_manager_set_update_gate below. */
typedef struct target_reacquire_c {
  int max_rejects;           /* K: 1..127 re-initialise on the K-th consecutive rejection; 0 count only */
  unsigned char* event_dev;  /* device memory or NULL: per tick, row [ld] of the bytes defined above */
  long ld;                   /* >= batch size (ignored when event_dev is NULL) */
  long tick_stride;          /* bytes between rows of consecutive ticks (>= ld); 0 = every tick overwrites one row */
  long ring_ticks;           /* as for the innovation stream */
} target_reacquire_c;
int target_batch_step_sequence_reacquire(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                         long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                         const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                                         const target_reacquire_c* reacq, int use_graph);
/* per_batch_reacq[i]: the policy of batch i (NULL: none for any batch); a batch without one passes max_rejects = -1 */
int target_manager_step_sequence_all_reacquire(target_manager_c* m, long n_ticks, double dt,
                                               const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                               const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max,
                                               const target_reacquire_c* per_batch_reacq, long n_batches,
                                               int query, const double* origin, double radius, int use_graph);
/* ---- The innovation stream, the gate and the re-acquisition INSIDE a temporally fused call.
 * target_batch_step_fused[_poses] with the streams and policies of the sections above: n_ticks ticks in ONE launch, each target's
 * state in registers across the ticks, and in every tick the two-phase gated body and the policy of ..._reacquire -- the
 * rejection run of a slot lives in a register from the call's first tick to its last (read once at the start, written back with
 * the records), and a lost target is re-initialised in registers.  For replaying a recorded stream WITH outliers.
 * EQUALITY.  For every slot and every tick the call equals target_batch_step_sequence_reacquire called with the same arguments,
 * ring_ticks = 0 for the measurements and use_graph = 0, bit for bit: state, covariance, unwrap memory, measurement counter,
 * clock, rejection runs, every NIS row, innovation block, event row and pose block.  `innov` and `reacq` keep their own
 * ring_ticks and their zero strides, with the meaning they have there; columns >= size are never written.
 *   reacq == NULL                      the semantics of ..._gated; the rejection runs are neither read nor written.
 *   nis_max == 0 with an innov         the plain innovation stream of ..._innov, from a fused call.
 *   nis_max == 0 and innov == NULL     exactly target_batch_step_fused_poses: the same kernels.
 *   meas_dev == NULL                   a predict-only call: NIS -1, zero innovations, runs unchanged; as in the ..._reacquire call
 *                                      (which launches no policy for such a tick) the event rows are not written.
 * REFUSED (negative return, target_manager_last_error, nothing launched or changed): what ..._reacquire, ..._gated and ..._innov
 * refuse -- a policy without a gate; a gate without the NIS row; max_rejects outside 0..127; nis_max < 0 or NaN; ld < size, a
 * stride in (0, ld) or negative, ring_ticks < 0 in either stream; a policy on a batch that keeps measured poses or that no longer
 * keeps its initial covariances -- and, for the call itself, n_ticks beyond an int, a negative tick_stride or has_stride, and
 * ld < size with measurements.
 * WHO SERVES IT.  One-class batches in the axis-separable layouts (lanes 201 and 301: the automatic layout of the shipped models),
 * fp64 and fp32, every model: one launch for the whole call (kf_step_sep_fused_gate_kernel), every instantiation at zero scratch
 * (profiles/fused_gate_kernel_resources.txt); none had to be routed tick by tick.  ..._step_fused_gate_served says 1 for these.
 * A shared-axes batch is expanded to the plain form first, as target_batch_step_fused does.  Served TICK BY TICK INSIDE THE CALL,
 * by the launches ..._reacquire makes for each tick -- same results, its launch counts -- and reported as 0: the dense layouts
 * (coupled Q / R / P0, an explicit lanes_per_target outside 201 / 301, the symmetric-packed EKF), batches with several (Q, R)
 * classes, batches that keep measured-pose rows.  A call WITH `poses` is served tick by tick as well, whatever ..._served says:
 * the fused gated kernels carry no pose block (chosen over a second set of instantiations; the bits are the same either way).
 * target_batch_step_fused and target_batch_step_fused_poses stay exactly as they are.
 * ..._step_fused_gate_served: 1 = one launch for the whole call (without `poses`); 0 = served tick by tick inside the call; -1 on error.
 * The same call for every batch of a manager at once: target_manager_step_fused_all below.
 * Not served: per-axis gates; M-of-N logic. */
int target_batch_step_fused_gated(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                                  const unsigned char* has_meas_dev, long has_stride,
                                  const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                                  const target_reacquire_c* reacq);
int target_batch_step_fused_gate_served(target_batch_c* b);   /* 1: one launch for the whole call; 0: served tick by tick inside the call */
/* ---- Step sequences and fused replays with a TIME STEP PER TICK (a time-step schedule).
 * A recorded stream has the stamps it has: jitter, a late frame, a dropped frame.  The calls below are the most general form of
 * each multi-tick family with `double dt` replaced by a host array dt_host[n_ticks]: tick s of the call runs with dt_host[s].
 *   ..._step_sequence_dt      follows target_batch_step_sequence_reacquire
 *   ..._step_fused_dt         follows target_batch_step_fused_gated
 *   ..._step_sequence_all_dt  follows target_manager_step_sequence_all_reacquire
 * poses, innov and reacq NULL with nis_max == 0 give the plain calls.  dt_host is read before the call returns.  Entries are taken
 * as target_batch_step takes its dt: no validation of values (0.0 is a tick that only updates).
 * CONTRACT.  For every slot the call equals n_ticks calls of its scalar-dt counterpart with n_ticks = 1 and dt = dt_host[s], the
 * measurement, mask and stream pointers moved to tick s -- bit for bit: state, covariance and unwrap memory; measurement counter
 * and rejection runs; every NIS row, innovation block, event row and pose block; the query outputs; and the target's time.  The
 * clock is therefore advanced by one compensated addition per tick, in order, as target_batch_step does -- never by dt * n.
 * A schedule whose entries are all equal gives the scalar call's bits everywhere EXCEPT the clock: the time read back may differ
 * from the scalar call's by at most 1 ulp (both are roundings of sums exact to about 2^-106: dt added n times there, dt * n here).
 * REFUSED (negative return, target_manager_last_error, nothing launched or changed): dt_host == NULL with n_ticks > 0, and
 * everything the scalar counterpart refuses.
 * RECORDED GRAPHS (use_graph = 1).  A recording bakes every tick's dt into its launch, so it is filed under the schedule's VALUES,
 * compared as bits (0.0 and -0.0 differ).  A replay with the same schedule reuses the recording -- a ring replayed in blocks
 * with a repeating schedule is such a case; a different schedule records anew.  A caller with a fresh schedule every call gains
 * nothing over use_graph = 0 (it records every time): the fused call is the form for that case.
 * WHO SERVES THE FUSED CALL.  One-class batches in the axis-separable layouts (lanes 201 and 301), fp64 and fp32, every model: one
 * launch for the whole call -- the fused loop (kf_step_sep_fused_dt_kernel) or, with an innovation stream, a gate or a policy, the
 * gated fused loop (kf_step_sep_fused_gate_dt_kernel) -- whose tick s reads entry s of a device table of doubles with one scalar
 * load.  The batch owns the table and fills it on its stream ahead of the launch; every call takes a fresh run of it, so calls
 * enqueued back to back without a synchronisation do not see each other's values.  Every instantiation has zero scratch
 * (profiles/dt_schedule_kernel_resources.txt); none had to be routed tick by tick.  ..._step_fused_dt_served says 1 for these.
 * Served TICK BY TICK INSIDE THE CALL, same results, reported as 0: a call with `poses`; the dense layouts and the
 * symmetric-packed EKF; several (Q, R) classes; batches that keep measured poses; a call of more than 2^28 ticks.  A shared-axes
 * batch is expanded to the plain form first, as for every fused call; it reports 0 until then (its first call is the expansion,
 * a synchronisation and then the plain form's launch) and what the plain form reports afterwards.
 * ..._step_fused_dt_served(b, gated): gated = the call would carry innov, nis_max > 0 or reacq.  1 = one launch for the whole call
 * (without `poses`); 0 = tick by tick inside the call; -1 on error.
 * OUT OF SCOPE.  Resident sessions keep the one dt of target_batch_live_start (a schedule there needs a hand-off of its own
 * through the ring and the clock kept on the device); a dt per target inside a dense tick (the by-id calls have one); the fused
 * kernel of the dense layouts stays as it is (such a batch's schedule call runs its single ticks). */
int target_batch_step_sequence_dt(target_batch_c* b, long n_ticks, const double* dt_host, const void* meas_dev, long tick_stride,
                                  long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                  const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                                  const target_reacquire_c* reacq, int use_graph);
int target_batch_step_fused_dt(target_batch_c* b, long n_ticks, const double* dt_host, const void* meas_dev, long tick_stride, long ld,
                               const unsigned char* has_meas_dev, long has_stride,
                               const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                               const target_reacquire_c* reacq);
int target_batch_step_fused_dt_served(target_batch_c* b, int gated);   /* 1: one launch for the whole call; 0: tick by tick inside the call; -1 error */
int target_manager_step_sequence_all_dt(target_manager_c* m, long n_ticks, const double* dt_host,
                                        const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                        const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max,
                                        const target_reacquire_c* per_batch_reacq, long n_batches,
                                        int query, const double* origin, double radius, int use_graph);
/* ---- ONE LAUNCH for a temporally fused replay of a WHOLE MANAGER.
 * The manager-level form of target_batch_step_fused_gated (..._all) and target_batch_step_fused_dt (..._all_dt): a manager with one
 * batch per motion model replays a recording of n_ticks ticks as one launch per device instead of one per batch.
 * per_batch [n_batches] in batch order (shard-major on several devices, as for ..._step_sequence_all); per_batch_poses,
 * per_batch_innov, per_batch_nis_max and per_batch_reacq [n_batches] may each be NULL (none for any batch), and an entry with
 * max_rejects < 0 in per_batch_reacq is no policy for that batch.  per_batch[i].ring_ticks must be 0 (fused calls read linearly);
 * delta_dev and pose_dev are ignored (fused calls have no query).
 * CONTRACT.  For every batch i the call equals target_batch_step_fused_gated (..._all_dt: target_batch_step_fused_dt) on batch i with
 * the same arguments, bit for bit: state, covariance and unwrap memory; measurement counters, clock and rejection runs; every NIS
 * row, innovation block, event row and pose block.
 * WHO SERVES IT.  ONE LAUNCH PER DEVICE (kf_step_population_fused_kernel: the grid of the population tick, each part the per-batch
 * fused loop of its model on its own arguments, every part reading the call's one time-step table) when all of these hold: at
 * least two non-empty batches, each a one-class batch of its own model in the axis-separable layout with packed groups (lanes 301,
 * fp64 or fp32; a shared-axes batch is expanded to the plain form first, as for every fused call); no batch has `poses` in the
 * call or keeps measured-pose rows; with a schedule, n_ticks <= 2^28; and either no batch carries a stream, a gate or a policy (the
 * plain loop) or every non-empty batch carries at least its NIS rows (the gated loop; nis_max per batch, 0 = that batch's plain
 * stream).  Every instantiation has zero scratch (profiles/fused_all_kernel_resources.txt).  EVERYTHING ELSE is served inside the
 * same call by the per-batch calls in batch order -- same bits, their launch counts: a single non-empty batch, the coupled or dense
 * layouts, several (Q, R) classes, a call in which only some batches carry streams, a call with `poses`, batches that keep
 * measured poses.
 * REFUSED (negative return, target_manager_last_error, NO batch launched or changed, its storage form included): a NULL manager;
 * n_batches other than the manager's number of batches; ring_ticks != 0; ..._all_dt with dt_host == NULL and n_ticks > 0; and, for
 * every batch, everything target_batch_step_fused_gated refuses -- ld < size with measurements also where that batch carries no
 * stream.
 * ..._served(m, gated, scheduled): gated = every batch would carry NIS rows; scheduled = the ..._all_dt form.  1 = one launch per
 * device for such a call without `poses`, as the batches are now; 0 = per batch inside the call; -1 on error. */
int target_manager_step_fused_all(target_manager_c* m, long n_ticks, double dt, const target_batch_sequence_c* per_batch,
                                  const target_pose_stream_c* per_batch_poses, const target_innov_stream_c* per_batch_innov,
                                  const double* per_batch_nis_max, const target_reacquire_c* per_batch_reacq, long n_batches);
int target_manager_step_fused_all_dt(target_manager_c* m, long n_ticks, const double* dt_host, const target_batch_sequence_c* per_batch,
                                     const target_pose_stream_c* per_batch_poses, const target_innov_stream_c* per_batch_innov,
                                     const double* per_batch_nis_max, const target_reacquire_c* per_batch_reacq, long n_batches);
int target_manager_step_fused_all_served(target_manager_c* m, int gated, int scheduled);   /* 1: one launch per device; 0: per batch inside the call; -1 error */
/* recordings made so far by the batch's step_sequence* calls with use_graph != 0 (a counter for tests of the graph cache); -1 on error */
long target_batch_graph_recordings(target_batch_c* b);
/* the rejection run of every slot, slot order, into runs_host [size]; synchronises */
int target_batch_rejection_runs(target_batch_c* b, unsigned char* runs_host);
/* the rejection run of one target: >= 0, or negative: unknown id */
int target_manager_get_rejection_run(target_manager_c* m, unsigned int id);
/* ---- The gate and the re-acquisition on the by-id and one-target paths: a sticky update policy.
 * The calls above serve callers whose loop is built around device-resident buffers.  A caller of the reference's own symbols --
 * target_manager_update_meas per target, or the two-call node tick target_manager_update_meas_batch + ..._get_est_batch of
 * examples/node_tick.c, or target_ingest_tick -- sets a POLICY once and keeps its loop: per manager and per model, off by
 * default, applied from then on to every call that steps targets BY ID WITH A MEASUREMENT: target_manager_update_meas,
 * target_manager_update_meas_batch, ..._update_meas_batch_gated below, target_ingest_tick and the Eigen facade's update.
 * target_batch_step*, the step_sequence* calls, target_batch_step_fused, the resident mode and target_manager_update_all keep
 * their own arguments and ignore the policy; a by-id step without a measurement is the plain predict-only step.
 * Per entry the semantics are exactly those of the dense calls: the decision is (double)NIS <= nis_max (a NaN rejects); an
 * accepted entry leaves in the bits of the ungated by-id step with a measurement, a rejected one in the bits of the ungated
 * by-id step without (state, covariance, unwrap memory, measurement counter); the clock advances by the entry's own dt either
 * way.  With max_rejects >= 0 the slot's rejection run -- the byte of the ..._reacquire section -- follows that section's table,
 * and a re-initialised slot's record is bit for bit the record a fresh target gets from this entry's measurement (v0 = a0 = 0,
 * the slot's own P0, unwrap memory 0; clock and counter untouched).  An id named twice in one call is two consecutive gated
 * steps; queued one-target steps with different dt are each gated with their own dt.
 * How: ONE launch per flush / indexed call, as without a policy -- the gated indexed step kernel carries the rejection-run
 * policy in its tail and still fills the getter table; a call that names exactly one batch's ids in slot order runs the dense
 * gated kernel and the re-acquisition launch of the sections above.
 * type: a model type (0 angular_rates, 1 angular_velocities, 2 uniform_acceleration, 3 uniform_velocity), or -1 = every model.
 * nis_max: 0 = no gate (default), > 0 (+inf included) = gated.  max_rejects: -1 = gate only (rejection runs untouched), 0 = count
 * only, 1..127 = re-initialise on the K-th consecutive rejection.  Flushes every queued one-target step first.  Applies to
 * batches created later too.
 * Refused with a negative code, target_manager_last_error set and NOTHING STEPPED IN THE WHOLE CALL: nis_max < 0 or NaN;
 * max_rejects outside -1..127; max_rejects >= 0 with nis_max == 0; a by-id update with measurements under a policy that touches a
 * batch with no gated indexed kernel (the dense layouts of coupled Q / R / P0 or an explicit lanes_per_target outside 201 / 301,
 * the symmetric-packed EKF, several (Q, R) classes, a batch that keeps measured-pose rows); for max_rejects >= 0, a batch that no
 * longer keeps its initial covariances.  target_manager_update_gate_served asks up front.  The void one-target symbol reports
 * through target_manager_last_error, as its other failures do.
 * Not served: the innovations nu by id (NIS only); per-class, dense-layout and keep-measurement batches by id.
 * (The resident mode and the fused calls ignore this policy and have gates of their own: target_batch_live_set_gate,
 * target_batch_step_fused_gated.) */
int  target_manager_set_update_gate(target_manager_c* m, int type, double nis_max, int max_rejects);
int  target_manager_get_update_gate(target_manager_c* m, int type, double* nis_max, int* max_rejects);
/* 1 if by-id updates of this model's batch would be served under a policy, 0 if not (see "refused"), -1 unknown */
int  target_manager_update_gate_served(target_manager_c* m, int type);
/* target_manager_update_meas_batch under the manager's policy, reporting per ENTRY i (caller's order):
 * nis_out[i] (or NULL): NIS of the measurement; -1 = no measurement on this entry (or no policy for its model: nothing was
 *   judged); -2 = unknown id (not stepped)
 * event_out[i] (or NULL): the event byte of target_reacquire_c's table (0 when max_rejects == -1)
 * Returns the number of targets stepped, after the outputs are in the caller's arrays. */
long target_manager_update_meas_batch_gated(target_manager_c* m, const unsigned int* ids, long n, double dt,
                                            const double* meas, const unsigned char* has_meas,
                                            double* nis_out, unsigned char* event_out);
/* Resident ("live") mode (target_batch_live_* above) for EVERY batch of a manager at once (BASELINE.json configs[3] / configs[4]: two motion models per GPU, whose per-GPU
 * share is launch-bound): one resident kernel per batch, each on a stream of its own so that they are on the device together;
 * per_batch[i] describes batch i's ring as for target_manager_step_sequence_all (ring_ticks > 0); with query != 0 the own-time
 * sphere query of every target runs after every tick inside the resident kernels, into per_batch[i].delta_dev / pose_dev
 * (overwritten every tick), as target_manager_step_sequence_all's fused query does; like the pose output above they are written
 * THROUGH the caches before the tick counts as done: copy them on another stream after ..._live_done_all reached tick k and they
 * hold the results of a tick >= k (exactly k when one tick is posted at a time).  The
 * sessions' wavefronts must fit the device together.  ..._post_all: n_ticks to every batch (one_doorbell_per_tick != 0: as
 * n_ticks separate doorbells); ..._done_all: ticks finished by every wavefront of every batch; ..._stop_all: ticks served. */
int target_manager_live_start_all(target_manager_c* m, double dt, const target_batch_sequence_c* per_batch, long n_batches, long first_entry,
                                  long max_ticks, double idle_limit_s, int query, const double* origin, double radius);
int target_manager_live_post_all(target_manager_c* m, long n_ticks, int one_doorbell_per_tick);
long target_manager_live_done_all(target_manager_c* m);
int target_manager_live_wait_all(target_manager_c* m, long tick, double timeout_s);
long target_manager_live_stop_all(target_manager_c* m);
/* derived outputs of every slot into device arrays of doubles ([size][7], [size][6], [size][6];
 * any may be NULL); at_time != 0 extrapolates to t1 */
int target_batch_get_est_dev(target_batch_c* b, double* pose_dev, double* twist_dev, double* acc_dev, int at_time, double t1);
/* every slot of the batch: delta_dev [size], pose_dev [size][7] or NULL (device doubles); a NaN t1
 * means "each target's own current time" (the per-tick fused query of BASELINE.json configs[4]);
 * origin is a host array of 3 */
int target_batch_intersect_sphere_dev(target_batch_c* b, double t1, const double* origin, double radius,
                                      double* delta_dev, double* pose_dev);
/* the gated form for every slot; delta_dev and pose_dev are required (the gate reads them) */
int target_batch_intersect_sphere_converged_dev(target_batch_c* b, double t1, double pos_th, double ang_th,
                                                const double* origin, double radius, int filters_length,
                                                double* delta_dev, double* pose_dev, unsigned char* converged_dev);
/* The convergence gate alone (IntersectionSolver::getIntersectionPoseWithSphere, src/intersection_solver.cpp:102-120),
 * fed with query results already on the device -- e.g. the delta / pose arrays the per-tick query of
 * target_manager_step_sequence_all leaves behind: delta_dev [size], pose_dev [size][7] -> converged_dev [size];
 * filtered_dev [size][2] (filtered position / angle error) and variance_dev [size][2]
 * (MovingAvgFilter::getVariance, utils.hpp:241-251; O(filters_length) per target, NULL skips it) are optional. */
int target_batch_gate_update_dev(target_batch_c* b, const double* delta_dev, const double* pose_dev, double pos_th, double ang_th,
                                 int filters_length, unsigned char* converged_dev, double* filtered_dev, double* variance_dev);
/* ---- THE k SOONEST CROSSINGS: a stream-ordered selection over query results already on the device.
 * What an interceptor asks of the delta [size] / pose [size][7] arrays a tick with the query leaves behind: which few targets
 * cross the sphere soonest, when, and where.  Inputs: delta_dev [size] and, or not, pose_dev [size][7] (device doubles, whatever
 * the batch precision) and ok_dev [size] (device bytes, e.g. the `converged` of target_batch_gate_update_dev; NULL: every slot).
 * CANDIDATES.  Slot i is a candidate iff (ok_dev == NULL || ok_dev[i] != 0) && delta[i] >= delta_lo && delta[i] <= delta_hi.  A NaN
 * delta is never one; the library's "no intersection" -1 is never one (delta_lo >= 0 is required); delta_hi may be +inf.
 * ORDER.  Ascending by delta compared as doubles (-0.0 == 0.0), ties by ascending slot; across a manager by (delta, batch index
 * in target_manager_get_batch order, slot).  Deterministic: the result is a function of the inputs alone.
 * RESULT.  count = min(k, number of candidates) rows in that order: the slot (and the batch index at manager level), delta as the
 * input's own bits and, with the pose pair, that slot's 7 pose words bit for bit.  Rows count .. k-1 are slot -1, batch -1,
 * delta -1, pose [0 0 0 0 0 0 1] (id 0xffffffff in the host forms).  1 <= k <= TARGET_SOONEST_MAX_K.
 * REFUSED (-1, target_manager_last_error, nothing enqueued, nothing written): k out of range; delta_lo < 0 or NaN; delta_hi <
 * delta_lo or NaN; a NULL delta_dev; a NULL output other than the pose pair; pose_out without pose_dev, or the reverse.  An empty
 * batch gives count 0 and k filler rows.  uniform_velocity and angular_velocities batches never intersect (all -1): nothing selected.
 * SLOTS are positions in the dense order (target_batch_slot_ids) and stay valid until the next erase or init of that batch; so
 * does a device result.  The host forms translate them to ids before they return.
 * The selection reads NO filter record: it settles no uniform tiles, expands no shared-axes batch, drops no recorded sequence and
 * does not run the queued one-target steps.  Three launches whatever size and k (a top-k per workgroup, then two merges;
 * DESIGN.md 3.16), no atomics, plain stores; TE_SELECT_SOONEST_MAX_WGS (default 1024, read when the manager is created) caps the
 * first launch's workgroups.
 *   ..._select_soonest_dev   enqueued on the batch's stream behind whatever produced the inputs there; no host synchronisation
 *                            and, after the device's first selection, no allocation: it may be captured in the caller's own
 *                            hipGraph behind target_manager_step_sequence_all(..., n_ticks = 1, query = 1, ...).  Outputs in
 *                            device memory: slot_out_dev int[k], delta_out_dev double[k], pose_out_dev double[k][7] or NULL,
 *                            count_out_dev int[1].
 *   ..._select_soonest       the same plus one small copy and a synchronisation; ids_out unsigned[k], slots_out int[k],
 *                            delta_out double[k], pose_out double[k][7] or NULL are host arrays.  Returns count (or -1).
 *   target_manager_select_soonest       every batch of the manager: per_batch [n_batches] is the array handed to
 *                            target_manager_step_sequence_all, of which only delta_dev and pose_dev are read (a NULL delta_dev
 *                            skips the batch); ok_dev_per_batch [n_batches] device pointers or NULL (an entry may be NULL).  Here
 *                            pose_out decides about the gather: with it every selected batch needs its pose_dev, without it the
 *                            pose_dev entries are not read.  All batches of a device are selected together by one set of
 *                            launches (at most 16 per device), the devices' rows merged on the host.  Everything is checked
 *                            before anything is enqueued on any device.  batch_out int[k].  Returns count (or -1).
 *   target_manager_select_soonest_dev   the device form for a manager on ONE device, on the manager's stream; refused on a manager
 *                            with several shards: there is no single device to leave the result on.
 * Not served: the selection as a per-tick stream inside recorded sequences, fused calls and resident sessions; ids on the device. */
#define TARGET_SOONEST_MAX_K 256
int target_batch_select_soonest_dev(target_batch_c* b, const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev,
                                    double delta_lo, double delta_hi, long k, int* slot_out_dev, double* delta_out_dev,
                                    double* pose_out_dev, int* count_out_dev);
long target_batch_select_soonest(target_batch_c* b, const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev,
                                 double delta_lo, double delta_hi, long k, unsigned int* ids_out, int* slots_out, double* delta_out,
                                 double* pose_out);
long target_manager_select_soonest(target_manager_c* m, const target_batch_sequence_c* per_batch, long n_batches,
                                   const unsigned char* const* ok_dev_per_batch, double delta_lo, double delta_hi, long k,
                                   unsigned int* ids_out, int* batch_out, int* slots_out, double* delta_out, double* pose_out);
int target_manager_select_soonest_dev(target_manager_c* m, const target_batch_sequence_c* per_batch, long n_batches,
                                      const unsigned char* const* ok_dev_per_batch, double delta_lo, double delta_hi, long k,
                                      int* batch_out_dev, int* slot_out_dev, double* delta_out_dev, double* pose_out_dev,
                                      int* count_out_dev);
/* ---- POSITION COVARIANCE AND TIME SPREAD AT A SPHERE CROSSING: how well a crossing is known, from the filter's own covariance.
 * For row i with delta[i] >= 0 (a query's time to the crossing) and its slot's state x, covariance P and class matrix Q:
 *   tau   = delta[i] + dq, dq the query's own offset: 0 for t1 = NaN (each target's own time), else t1 - the target's time
 *   Sigma = (A(tau) P A(tau)^T + Q)[0:3, 0:3], the position block a predict-only update(dt = tau) of the reference would leave (Q
 *           added once, as every predict does), in the batch's precision and in the predict's statement order of the step kernels.
 *           Only the position chains {r, r + K, (r + 2K)}, r = 0..2, enter; in the axis-separable layouts the off-diagonal entries
 *           are exact zeros, and a shared-axes batch has three equal diagonal entries.
 *   cov_out [n][6] = the upper triangle of Sigma: xx xy xz yy yz zz.
 * With origin (host double[3]; radius > 0 is checked, the query that made delta used it), in double: p_c, v_c = position and linear
 * velocity at tau as the query extrapolates them, n = (p_c - o) / |p_c - o|,
 *   sigma_out [n][2] = { sigma_r = sqrt(n^T Sigma n), sigma_t = sigma_r / |n . v_c| } -- the spread of the position along the
 *           sphere's normal, and to first order of the crossing time; sigma_t = +inf when n . v_c == 0.  Nothing is clamped: a
 *           negative form or |p_c - o| == 0 gives NaN.
 *   ok_out [n]       = delta >= 0 && sigma_r <= sigma_r_max && sigma_t <= sigma_t_max (<=: a NaN rejects; a bound may be +inf) --
 *           a mask for target_batch_select_soonest_dev.
 * NON-CANDIDATES.  A row whose delta is negative or NaN, or whose slot is -1 (or outside the batch), gets cov 0, sigma {-1, -1},
 * ok 0, and costs no record word: its delta is all that is read.
 * ROWS.  slots_dev == NULL: dense, row i is slot i, n <= size.  Else slots_dev int[n] (device), n <= TARGET_CROSSING_COV_MAX_ROWS,
 * delta_dev [n] by row -- the slot_out_dev / delta_out_dev of a selection.  At manager level batch_dev int[n] runs alongside (the
 * batch_out_dev of target_manager_select_soonest_dev): every batch's launch serves its rows, every row is written exactly once.
 * REFUSED (-1, target_manager_last_error, nothing enqueued, nothing written): a NULL delta or cov_out; sigma_out or ok_out without
 * origin; radius <= 0 or NaN with origin; a NaN threshold; n < 0 or beyond the form's limit; the manager's device form on a
 * manager with several shards.
 * The call reads the records as they are stored (a uniform tile's words from the tile's block): it settles no tile, expands no
 * shared-axes batch, drops no recorded sequence and leaves rejection runs and clocks alone; the queued one-target steps run first.
 *   ..._crossing_cov_dev     one launch per batch on its stream, no allocation, no host synchronisation: it may be captured in
 *                            the caller's hipGraph behind target_manager_step_sequence_all(..., n_ticks = 1, query = 1, ...) and a
 *                            selection.  All arrays but origin in device memory.
 *   target_manager_crossing_cov_batch   by id with host arrays (delta_host [n], e.g. of target_manager_get_intersection_batch), any
 *                            number of ids over any number of shards; an unknown id gets the non-candidate row.  Returns the
 *                            number of ids found (or -1).
 * Not served: the Eigen facade; a per-tick stream of these rows inside recorded sequences, fused calls and resident sessions. */
#define TARGET_CROSSING_COV_MAX_ROWS 8192
int target_batch_crossing_cov_dev(target_batch_c* b, double t1, const double* origin, double radius, const double* delta_dev,
                                  const int* slots_dev, long n, double sigma_r_max, double sigma_t_max, double* cov_out_dev,
                                  double* sigma_out_dev, unsigned char* ok_out_dev);
int target_manager_crossing_cov_dev(target_manager_c* m, double t1, const double* origin, double radius, const int* batch_dev,
                                    const int* slots_dev, const double* delta_dev, long n, double sigma_r_max, double sigma_t_max,
                                    double* cov_out_dev, double* sigma_out_dev, unsigned char* ok_out_dev);
long target_manager_crossing_cov_batch(target_manager_c* m, const unsigned int* ids, long n, double t1, const double* origin, double radius,
                                       const double* delta_host, double sigma_r_max, double sigma_t_max, double* cov_out,
                                       double* sigma_out, unsigned char* ok_out);
/* ---- ASSOCIATION OF UNLABELLED DETECTIONS: a frame of M detections without target labels is paired with the targets of a batch (or
 * of a whole manager on ONE device) on the device, from the filter's own predicted positions and innovation covariances, and
 * scattered into the form the tick reads.  
 * INPUTS.  dt: the time step of the tick that will consume the result.  det [M][7] doubles in the reference's pose layout
 * [x y z qx qy qz qw].  gate > 0 (may be +inf).  rounds: 1 .. TARGET_ASSOC_MAX_ROUNDS.
 * PER TARGET (slot), whatever its model:
 *   zhat  = the position a predict-only update(dt) would give, as the getters extrapolate it to the offset dt, in the batch's precision
 *   Sigma = (A(dt) P A(dt)^T + Q)[0:3, 0:3] exactly as target_batch_crossing_cov_dev forms it at tau = dt: the batch's precision, the
 *           stored words (a uniform tile's from the tile's block), exact zeros between the axes of the separable layouts
 *   S     = Sigma + R[0:3, 0:3], R of the slot's own (Q, R) class, summed in double
 *   W     = S^-1 in double, by cofactors: symmetric, 6 words.  A slot whose S is not finite, has a non-positive diagonal entry or a
 *           non-positive determinant is never a candidate.
 * PAIR COST.  d2(i, j) = nu^T W_i nu, nu = det_j[0:3] - zhat_i, in double; (i, j) is a candidate iff d2 <= gate, so a NaN in either
 * operand rejects the pair.  POSITION ONLY, for all four models: a detection's orientation is not used for pairing.  The angular
 * models' full 6-dof NIS is still applied afterwards by the tick's own gate, if one is set.
 * MATCHING, in rounds of mutual best: every unmatched target picks its best unmatched candidate detection by (d2, detection index),
 * every unmatched detection its best unmatched candidate target by (d2, batch index, slot); a pair that picked each other is
 * matched; the next round repeats on what is left.  At its fixed point this is greedy global-nearest-neighbour: take the smallest
 * remaining pair by (d2, batch, slot, detection), remove its row and column, repeat.  The result is a function of the inputs alone.
 * ROUNDS.  A round is settled if every unmatched detection that had a candidate at its start was matched in it (also: none had
 * one).  After a settled round no pair remains; the launches of later rounds return at once.  info[2] = 1 guarantees the greedy
 * result, 0 means that more rounds might add matches.
 * OUTPUTS.  meas_out SoA [7][ld] in the batch precision and has_meas_out [size] bytes, as target_batch_step reads them: a matched
 * slot gets its detection's 7 words rounded once and 1, an unmatched slot [0 0 0 0 0 0 1] and 0.  det_of_slot int[size] (-1: none),
 * d2_of_slot double[size] (-1: none); slot_of_det int[M] (and batch_of_det int[M] at manager level), d2_of_det double[M] (-1: none).
 * d2_of_slot comes from the target-major scan, d2_of_det from the detection-major one: the same bits for a matched pair.
 * info int[4] = {matched, rounds_run, settled, 0}.  Required: meas_out, has_meas_out, info (device forms); the others may be NULL.
 * REFUSED (-1, target_manager_last_error, nothing enqueued, nothing written): a NULL handle; a NULL required output; M < 0 or
 * M > TARGET_ASSOC_MAX_DETECTIONS; det NULL with M > 0; ld < size; rounds out of range; gate <= 0 or NaN; dt negative or NaN; a
 * manager form on a manager with several shards.  M == 0 or an empty batch is no error: nothing matched, info = {0, 0, 1, 0}.
 * The call reads the records as they are stored: it settles no uniform tile, expands no shared-axes batch, drops no recorded
 * sequence and leaves rejection runs and clocks alone; the queued one-target steps run first.
 *   ..._associate_dev   everything in device memory, on the batch's (manager's) stream.  After the first call of at least that size
 *                       on a device it allocates nothing, and it never waits on the host: associate -> target_batch_step, or
 *                       associate -> target_manager_step_sequence_all(n_ticks = 1), may be captured in the caller's hipGraph.
 *   ..._associate       detections from host memory; the per-detection rows come back with slots translated to ids (~0u: none);
 *                       unmatched_out [M] receives the unmatched detection indices in ascending order, *n_unmatched_out their
 *                       number.  The device outputs (meas_out_dev ...) are optional here.  Returns the matched count (or -1).
 * These four scan all pairs by brute force; the ..._associate_grid forms below pair through a uniform grid.
 * Not built: orientation in the cost, a likelihood cost, several shards. */
#define TARGET_ASSOC_MAX_DETECTIONS 65536
#define TARGET_ASSOC_MAX_ROUNDS 16
/* what one batch's slots get from a manager-level call: one per batch, in target_manager_get_batch order */
typedef struct target_assoc_out_c {
  void* meas_out_dev;               /* SoA [7][ld] in the batch precision */
  long ld;
  unsigned char* has_meas_out_dev;  /* [size] */
  int* det_of_slot_dev;             /* [size] or NULL */
  double* d2_of_slot_dev;           /* [size] or NULL */
} target_assoc_out_c;
int target_batch_associate_dev(target_batch_c* b, double dt, const double* det_dev, long M, double gate, int rounds, void* meas_out_dev,
                               long ld, unsigned char* has_meas_out_dev, int* det_of_slot_dev, double* d2_of_slot_dev,
                               int* slot_of_det_dev, double* d2_of_det_dev, int* info_dev);
long target_batch_associate(target_batch_c* b, double dt, const double* det_host, long M, double gate, int rounds, void* meas_out_dev,
                            long ld, unsigned char* has_meas_out_dev, unsigned int* ids_of_det_out, int* slot_of_det_out,
                            double* d2_of_det_out, long* unmatched_out, long* n_unmatched_out, int* info_out);
int target_manager_associate_dev(target_manager_c* m, double dt, const double* det_dev, long M, double gate, int rounds,
                                 const target_assoc_out_c* per_batch, long n_batches, int* slot_of_det_dev, int* batch_of_det_dev,
                                 double* d2_of_det_dev, int* info_dev);
long target_manager_associate(target_manager_c* m, double dt, const double* det_host, long M, double gate, int rounds,
                              const target_assoc_out_c* per_batch, long n_batches, unsigned int* ids_of_det_out, int* batch_of_det_out,
                              int* slot_of_det_out, double* d2_of_det_out, long* unmatched_out, long* n_unmatched_out, int* info_out);
/* ---- THE GRID FORM of the association: the same pairing for full frames -- up to TARGET_ASSOC_GRID_MAX_DETECTIONS detections
 * against whatever the batch or manager holds -- through a uniform grid of cubic cells of edge `cell` (in the unit of the
 * positions), so that the cost grows with the pairs that are near each other and not with N x M.    The argument
 * lists are the brute-force siblings' plus `double cell` right after `rounds`; outputs, layouts, scatter, the host forms' id
 * translation and unmatched_out are the siblings'.  The table row (zhat, W, tag), the inverse of S, d2, the rounds of mutual best,
 * the settled rule and the tie rules -- (d2, detection) for a target's pick, (d2, batch, slot) for a detection's -- are the ones
 * above.  TWO THINGS DIFFER.
 * 1. THE CANDIDATE RULE GAINS THE GATE'S BOUNDING BOX: (i, j) is a candidate iff d2 <= gate AND nu_a * nu_a <= reach2_a(i) for each
 *    axis a of x, y, z, with reach2_a = (gate * S_aa) * (1 + 2^-10), S_aa the diagonal of the very S that was inverted, in double,
 *    nu_a the double that d2 is formed from; plain multiplies, no contraction, no square root.  In exact arithmetic the box
 *    contains the gate ellipsoid (nu_a^2 <= d2 S_aa), so the grid form differs from the brute-force form only where rounding in
 *    d2 exceeds one part in 10^3 of the gate -- a nearly singular S -- and it never accepts a pair that the brute-force form rejects.
 * 2. gate MUST BE FINITE (the box is what bounds the search).
 * CELLS.  A position's cell coordinate per axis is floor(x / cell) in double, clamped to [-2^30, 2^30].  A detection with a
 * non-finite position is binned nowhere and is never a candidate.  A valid slot is NARROW iff reach2_a <= (cell (1 - 2^-20))^2 on
 * all three axes (and that square is a normal double): all its candidates then lie within +-1 cell of the cell of zhat on each
 * axis, and are found by walking 27 cells.  Any other valid slot is WIDE: its candidates are found by brute force over all
 * detections -- correct, not fast.  info int[4] = {matched, rounds_run, settled, WIDE SLOTS}: a large info[3] says that cell is
 * too small for the targets' uncertainty.  A slot with an invalid S is neither.  Cells hash into a power-of-two number of
 * buckets (at least twice the entries binned, at least 1024; TE_ASSOC_GRID_BUCKETS, read when the manager is created, forces the
 * number for tests); collisions cost time, never correctness.
 * The result is a function of the inputs alone: two calls on the same inputs give byte-identical outputs.
 * REFUSED, in addition to the siblings' refusals (M against TARGET_ASSOC_GRID_MAX_DETECTIONS): gate +inf or NaN; cell <= 0, NaN or
 * inf.  ..._associate_grid_dev allocates nothing after the first call of at least that size, never waits on the host, and
 * associate_grid -> step may be captured in the caller's hipGraph (a linear chain of kernel launches), like the sibling.
 * Not built: orientation in the cost, a likelihood cost, several shards, per-tick association streams, the Eigen facade's form, an
 * automatic choice of cell. */
#define TARGET_ASSOC_GRID_MAX_DETECTIONS 1048576
int target_batch_associate_grid_dev(target_batch_c* b, double dt, const double* det_dev, long M, double gate, int rounds, double cell,
                                    void* meas_out_dev, long ld, unsigned char* has_meas_out_dev, int* det_of_slot_dev,
                                    double* d2_of_slot_dev, int* slot_of_det_dev, double* d2_of_det_dev, int* info_dev);
long target_batch_associate_grid(target_batch_c* b, double dt, const double* det_host, long M, double gate, int rounds, double cell,
                                 void* meas_out_dev, long ld, unsigned char* has_meas_out_dev, unsigned int* ids_of_det_out,
                                 int* slot_of_det_out, double* d2_of_det_out, long* unmatched_out, long* n_unmatched_out, int* info_out);
int target_manager_associate_grid_dev(target_manager_c* m, double dt, const double* det_dev, long M, double gate, int rounds, double cell,
                                      const target_assoc_out_c* per_batch, long n_batches, int* slot_of_det_dev, int* batch_of_det_dev,
                                      double* d2_of_det_dev, int* info_dev);
long target_manager_associate_grid(target_manager_c* m, double dt, const double* det_host, long M, double gate, int rounds, double cell,
                                   const target_assoc_out_c* per_batch, long n_batches, unsigned int* ids_of_det_out,
                                   int* batch_of_det_out, int* slot_of_det_out, double* d2_of_det_out, long* unmatched_out,
                                   long* n_unmatched_out, int* info_out);
/* ---- TRACK LIFECYCLE: start and retire targets from an association's results, on the device.    The unlabelled
 * path's counterpart of what target_ingest_* does for labelled measurements: a detection that matched nothing becomes a target, a
 * target that nothing has matched for max_misses frames goes away.  Only counts, the retired slots and the new ids cross the bus.
 * ORDER: associate -> step -> lifecycle.  Call it AFTER the tick that consumed the association: the lifecycle moves slots, so the
 * meas_out / has_meas_out columns of that association are STALE afterwards and must not be stepped again.
 * INPUTS, all device memory, all left untouched: det_dev [M][7] the frame; slot_of_det_dev [M] (< 0: unmatched) as
 * target_manager_associate[_grid]_dev wrote it; has_meas_dev [n_batches] one pointer per batch in target_manager_get_batch order,
 * the has_meas_out_dev [size] mask of the same target_assoc_out_c array (1: this slot was matched in this frame).  A caller on the
 * labelled path who builds the masks itself may use the retirement half alone (M = 0).
 * COUNTERS, two bytes per slot, library-owned like the rejection runs: miss = the run of consecutive lifecycle calls in which the
 * slot's mask byte was 0 (reset by a 1, saturates at 255); hits = the calls with a 1 since creation (saturates at 255).  Both are 0
 * at creation, however the target was created; both follow their target through every erase and through growth; only lifecycle
 * calls write them.  target_batch_track_counts copies them out (slot order; either array may be NULL; synchronises like
 * target_batch_rejection_runs); target_manager_get_track_counts returns 0 and one target's pair, 1 for an unknown id.
 * RULE.  The result is a function of the inputs alone.
 * 1. Every slot of every batch: miss and hits are updated from the mask.  A slot is STALE iff max_misses >= 1 and its new miss >=
 *    max_misses.  max_misses = 0 retires nobody; the counters are still kept.
 * 2. Detection j is BORN iff birth_type >= 0, slot_of_det[j] < 0, all seven words of its row are finite, and its rank among such
 *    detections, in ascending j, is < max_births (the lowest detection indices win).
 * 3. Retirements first: per batch the stale slots are erased as target_manager_erase_batch erases them given the ascending list
 *    (holes below the new size are filled, in order, by the survivors at or above it).
 * 4. Then births, appended in ascending j to the batch target_manager_init_batch_typed(birth_type, ...) would put them in (created
 *    if need be): born target j gets the id first_id + j and, bit for bit, the record that call creates from p0 = det[j],
 *    v0 = a0 = NULL, t0 = t_birth, dt0, Q, R, P0 with per_target_P0 = 0.  Q = R = P0 = NULL means the manager's own model
 *    parameters, allowed only when birth_type is the manager's default model.
 * OUTPUTS, host memory: retired_ids_out [retired_cap] the ids that went away, per batch in batch order, ascending former slot;
 * info long[6] = {retired, born, unmatched detections not born because of the cap, unmatched detections not born because
 * non-finite, first new id, one past the last new id}.  Returns 0, or -1 with target_manager_last_error.
 * REFUSED, and NOTHING CHANGES on a refusal (counters, records, ids, sizes): a NULL handle, policy or info; M < 0 or
 * M > TARGET_ASSOC_GRID_MAX_DETECTIONS; det or slot_of_det NULL with M > 0 and births on; n_batches != target_manager_num_batches; a
 * NULL mask for a non-empty batch; max_misses outside 0..255; birth_type outside -1..3; max_births < 0; NaN t_birth or dt0; only
 * some of Q, R, P0 given; the manager's parameters asked for a model that is not its default; a manager with several shards;
 * retired_cap smaller than the number retired; an id of [first_id, first_id + born) already in the manager, or that range
 * wrapping past 2^32 - 1.  What needs no handle is refused before the handle is looked at.  The plan is formed in scratch memory
 * and read back before anything is committed, so the refusals that depend on it change nothing either.
 * The call WAITS ON THE HOST and changes sizes: it is NOT CAPTURABLE in a hipGraph, and it does what erase and init already do to
 * recorded sequences, uniform tiles, shared-axes batches and live sessions.  Queued one-target steps and inits run first.
 * Not built: merging several unmatched detections of one new object AT BIRTH (the duplicate tracks that follow are found and retired
 * by target_manager_retire_duplicates below); a time-based (seconds) expiry; a confirmed-only mask for the
 * getters; several shards; the Eigen facade. */
typedef struct target_lifecycle_c {
  int max_misses;          /* K >= 1: retire on the K-th consecutive frame without a match; 0: retire nobody */
  int birth_type;          /* motion model 0..3 of new targets; -1: no births */
  unsigned int first_id;   /* born target j, in ascending detection index, gets first_id + j */
  long max_births;         /* cap per call */
  double dt0;              /* as target_manager_init_batch_typed */
  double t_birth;          /* its t0 */
  const double* Q;         /* as target_manager_init_batch_typed with per_target_P0 = 0; all three NULL: the manager's own */
  const double* R;
  const double* P0;
} target_lifecycle_c;
int target_manager_lifecycle(target_manager_c* m, const double* det_dev, const int* slot_of_det_dev, long M,
                             const unsigned char* const* has_meas_dev, long n_batches, const target_lifecycle_c* policy,
                             unsigned int* retired_ids_out, long retired_cap, long* info);
int target_batch_track_counts(target_batch_c* b, unsigned char* miss_host, unsigned char* hits_host);
int target_manager_get_track_counts(target_manager_c* m, unsigned int id, int* miss, int* hits);
/* ---- DUPLICATE TRACKS: find, and retire, two tracks that follow the same object, on the device.    A detector that
 * splits one object into two detections, or clutter next to a real target, gives birth to a second track inside the first one's
 * gate; the greedy one-to-one pairing then lets the two take turns, so neither ever reaches max_misses.  This is the self-join of
 * the association: row against row instead of row against detection, through the same uniform grid.  A manager on ONE device.
 * ROW.  Each slot of each batch gets one row, concatenated in target_manager_get_batch order.  zhat is exactly the association's
 * zhat at the offset dt; Sigma = (A(dt) P A(dt)^T + Q)[0:3, 0:3], the very doubles the association forms BEFORE it adds R (the same
 * accessors, uniform-tile words and exact zeros between separable axes).  A row is VALID iff the association's row is valid
 * (S = Sigma + R inverts) and Sigma's six words are finite: one validity rule.
 * ELIGIBLE.  A valid row is eligible iff its hits counter (TRACK LIFECYCLE above) is >= min_hits (0 .. 255) -- so that newborn
 * tracks, whose P0 covers everything nearby, are not called duplicates -- and it is NARROW: reach2_a = (gate * 2 Sigma_aa) *
 * (1 + 2^-10) <= (cell (1 - 2^-20))^2 on all three axes.  A valid row with enough hits that is not narrow is WIDE: it is EXCLUDED, not
 * brute-forced -- a track whose box exceeds a cell is not known well enough to be merged -- and counted in info[3]; a large info[3]
 * means that cell is too small.
 * PAIR.  For eligible rows lo < hi (row index): C = Sigma_lo + Sigma_hi word by word in double; V = C^-1 by the association's
 * cofactor inverse, an invalid C rejects the pair; d2 = nu^T V nu, nu = zhat_hi - zhat_lo.  The pair is a candidate iff d2 <= gate
 * AND nu_a * nu_a <= (gate * C_aa) * (1 + 2^-10) on every axis; plain multiplies, no contraction, no square root.  The pair's box
 * never exceeds the larger of the two rows' boxes, so a partner lies within +-1 cell and 27 cells suffice.  Both partners form the
 * same bits because both order the pair as (lo, hi).
 * MATCHING, in rounds of mutual best as the association's: every unmatched eligible row picks its best unmatched candidate partner
 * by (d2, partner row), never itself; two rows that picked each other are a pair.  rounds: 1 .. TARGET_ASSOC_MAX_ROUNDS; a round is
 * settled if every row that had a candidate at its start was matched in it; the launches of later rounds return at once.  The
 * fixed point is sorted greedy matching by (d2, lo, hi).
 * SURVIVOR.  Of a matched pair the WEAKER row is the duplicate: fewer hits; at equal hits, more miss; at equal both, the higher row.
 * A chain A-B-C therefore loses one track per call; the next frame's call sees the rest.
 * The result is a function of the inputs alone: two calls on the same inputs give byte-identical outputs.
 *   ..._find_duplicates_dev   on the manager's stream; reads the records and counters as stored and writes only its outputs.  After
 *                             the first call of at least that size it allocates nothing, never waits on the host and may be
 *                             captured in the caller's hipGraph.  dup_out_dev [size] per batch is required (1 = this slot is the
 *                             weaker of a matched pair); partner (batch, slot) and d2 (-1: none) are optional.  info int[4] =
 *                             {pairs, rounds_run, settled, wide rows}; an empty manager gives {0, 0, 1, 0}.
 *   ..._retire_duplicates     queued one-target work runs first; the same search into scratch memory; each batch's mask compacted
 *                             in ascending slot order; the counts, then the lists with their partners read back; both sides
 *                             translated to ids BEFORE anything moves; cap checked; only then are the duplicates erased as
 *                             target_manager_erase_batch erases them.  retired_ids_out [cap] / kept_ids_out [cap]: the duplicate
 *                             and the track that stays, per batch in batch order, ascending former slot.  info long[4] =
 *                             {retired, rounds_run, settled, wide}.  It WAITS ON THE HOST and is NOT CAPTURABLE, and it does to
 *                             recorded sequences, uniform tiles, shared-axes batches and live sessions what erase does.  Every
 *                             surviving target keeps its counters, its rejection run and its record bit for bit.  Call it when
 *                             slots are stable, for instance after the lifecycle: an earlier association's columns are STALE afterwards.
 * REFUSED (-1, target_manager_last_error, nothing enqueued, nothing written; NOTHING CHANGES on a refusal): a NULL handle; a NULL
 * info; a NULL dup_out_dev for a non-empty batch; n_batches != target_manager_num_batches; dt negative or NaN; gate <= 0, NaN or inf;
 * cell <= 0, NaN or inf; rounds out of range; min_hits outside 0 .. 255; cap < 0 or smaller than the number to retire; NULL id
 * arrays with cap > 0; a manager with several shards.  What needs no handle is refused before the handle is looked at.  (A cap
 * smaller than the number to retire is known only after the search: the queued one-target work has run by then, as it would have
 * on its own at the next call that reads the records; the population, records, ids and counters are untouched.)
 * Not built: fusing the two estimates instead of dropping one; brute force for wide rows; several shards; orientation in the cost;
 * the Eigen facade. */
typedef struct target_dup_out_c {       /* one per batch, target_manager_get_batch order */
  unsigned char* dup_out_dev;           /* [size] required: 1 = this slot is the weaker of a matched pair */
  int* partner_batch_dev;               /* [size] or NULL, -1: none */
  int* partner_slot_dev;                /* [size] or NULL, -1: none */
  double* d2_of_slot_dev;               /* [size] or NULL, -1: none; the same bits for both partners */
} target_dup_out_c;
int target_manager_find_duplicates_dev(target_manager_c* m, double dt, double gate, int rounds, double cell, int min_hits,
                                       const target_dup_out_c* per_batch, long n_batches, int* info_dev);
int target_manager_retire_duplicates(target_manager_c* m, double dt, double gate, int rounds, double cell, int min_hits,
                                     unsigned int* retired_ids_out, unsigned int* kept_ids_out, long cap, long* info);
/* AoS doubles [n][7] (host layout of the reference) -> SoA [7][ld] in the batch precision, on device */
int target_batch_pack_meas_dev(target_batch_c* b, const double* meas_aos_dev, long n, void* meas_soa_dev, long ld);

/* ---- synthetic measurement streams (SURVEY 8d "Synthetic inputs") ------------------------------------------ */
/* Counter-based generator: every number is a pure function of (seed, target, tick, component) -- splitmix64 keys, Box-Muller
 * normals with fixed-sequence log / sin / cos -- so the GPU fills its measurement ring with one kernel and a CPU checker
 * regenerates the same doubles bit for bit (csrc/stream_gen.hpp has the definition; it widens the generator of the
 * reference's integration test, test/target_manager_test.cpp:82-115, to a population: per-target start, velocity,
 * acceleration (uniform_acceleration), body rate; xyz + N(0, 0.01^2); quaternion = Qtran(dt, omega)^(tick+1) applied to the
 * identity).  Target i of a call is target first_target + i of the stream (ranks of a sharded run pass their offset).
 *   availability < 1 : a target has a measurement on a tick with that probability (has_meas_dev receives the bytes)
 *   rpy_noise  > 0   : the measured orientation is the true one times a small random rotation (rad, per axis) */
typedef struct target_stream_c {
  int model;                 /* TARGET_* motion model */
  unsigned long long seed;
  long first_target;
  double dt;                 /* tick length: tick s is time (s + 1) dt */
  double availability;       /* 1 = every target measured on every tick */
  double rpy_noise;          /* 0 = noiseless quaternion, as in the reference's test */
} target_stream_c;
/* ticks first_tick .. first_tick + n_ticks - 1 for n_targets targets: meas_dev = SoA ring [n_ticks][7][ld] (tick_stride
 * elements between ticks) in precision dtype (TARGET_DTYPE_*; values are generated in double and rounded once);
 * has_meas_dev [n_ticks][has_stride] bytes or NULL.  Asynchronous on hip_stream. */
int target_stream_fill_dev(const target_stream_c* spec, long n_targets, long first_tick, long n_ticks, int dtype, void* meas_dev,
                           long tick_stride, long ld, unsigned char* has_meas_dev, long has_stride, void* hip_stream);
/* pose0_dev [n][7]: the pose to create target i with (start position + measurement noise, identity orientation);
 * truth_dev [n][12]: p, v, a, omega of the generating motion.  Either may be NULL.  Device doubles. */
int target_stream_truth_dev(const target_stream_c* spec, long n_targets, double* pose0_dev, double* truth_dev, void* hip_stream);

/* ---- one manager over several devices ------------------------------------ */
/* target_manager_set_devices: give the manager n shards, shard k on HIP device devices[k] (repeats allowed: {0,0,0} is three
 * shards on device 0).  Call it after target_manager_new[_ex] and before the first target is created.  Every shard is a
 * complete manager on its device; the handle reaches all of them and every manager-level call above and below keeps its
 * signature and meaning (the ten reference symbols, init / update / erase / getters by id, the intersection calls and the
 * solver object, ingest, target_manager_population_tick, target_manager_step_sequence_all[_poses], synchronize).
 * Placement: a single creation goes to the shard with the fewest targets of its model (ties: lowest index); a batched
 * creation is cut into contiguous runs, in the caller's order, that fill the shards towards equal per-model counts; an
 * erased id created again is placed by the rule as it stands then.  n == 1 on the creation device: an unsharded manager.
 * Returns -1 (target_manager_last_error set, manager unchanged) if the manager already holds targets, n < 1, a device
 * index is out of range, or a stream was set with target_manager_set_stream (a stream belongs to one device: set the shards'
 * streams with target_manager_set_shard_stream).  target_manager_log decides its selection once for the whole manager (an
 * explicit list, or every target while the MANAGER holds at most 64) and writes the files an unsharded manager writes.  Where the shards span distinct devices, peer access between them is enabled here.
 * target_manager_num_batches / target_manager_get_batch enumerate the batches of every shard, shard-major, and the
 * per-batch specs of target_manager_step_sequence_all[_poses] follow that order: each spec's device pointers live on that
 * batch's device (target_manager_batch_shard, target_manager_shard_device).  Host-array calls split their ids by shard
 * and return the results in the caller's order; target_manager_get_available_targets stays ascending across shards.
 * REFUSED on a manager with more than one shard (-1 / NULL and a message, nothing launched): resident mode
 * (target_manager_live_*_all), the RCCL gather (target_manager_gather_pose_*), target_manager_set_stream (use
 * target_manager_set_shard_stream) and target_manager_get_batch_of_type (a model has one batch per shard, none of which holds
 * all its targets: use target_manager_get_batch with target_manager_batch_shard).  By default every shard launches on its
 * device's default stream. */
int target_manager_set_devices(target_manager_c* m, const int* devices, int n);
/* 1 for an unsharded manager */
int target_manager_num_shards(target_manager_c* m);
/* HIP device of shard k, -1 if there is no such shard */
int target_manager_shard_device(target_manager_c* m, int k);
/* shard that holds id, -1 for an unknown id */
int target_manager_shard_of(target_manager_c* m, unsigned int id);
/* shard of batch i (target_manager_get_batch order), -1 if there is no such batch */
int target_manager_batch_shard(target_manager_c* m, int index);
/* the stream (hipStream_t on shard k's device; NULL = that device's default stream) of shard k's launches */
int target_manager_set_shard_stream(target_manager_c* m, int k, void* hip_stream);
/* pose7 of every target in ascending id order -- the order of target_manager_get_available_targets -- into pose_out
 * [size][7] doubles: what the reference's node publishes every tick (src/target_manager_ros.cpp:78-87), for the whole
 * manager, without an id list.  pose_out is pinned host memory (hipHostMalloc or registered) or device memory that every
 * shard's device can reach.  One launch per batch (each target's pose by the getters' arithmetic, stored at its row);
 * asynchronous: the rows are complete when target_manager_synchronize returns.  The first call after a change of membership
 * (init, erase) rebuilds the per-batch row maps on the host, O(size log size), and uploads them stream-ordered through pinned
 * staging; it waits on the host only where a map has to grow (for the work still queued on that batch's stream).  pose_out == NULL only counts.  Works on
 * unsharded managers too.  Returns the number of rows (size), or -1 (capacity < size). */
long target_manager_get_est_all_by_id(target_manager_c* m, double* pose_out, long capacity);

/* ---- multi-GPU: gather of the estimated poses to one rank over xGMI (RCCL) ---------------------------- */
/* One process per GPU, every rank owns a shard of the targets (no collective in the predict/update path).  What the
 * reference's node does with the filtered poses every tick is publish them (src/target_manager_ros.cpp:78-87); across
 * GPUs that is a gather of pose7 rows to one rank.  It is a direct gather (one ncclSend per rank, one ncclRecv per peer
 * on the root: xGMI is point-to-point) on the communicator's own stream behind an event, so the step kernels of the
 * following ticks run while the poses travel.
 *   target_comm_unique_id : rank 0 creates the 128-byte id; the caller hands it to every rank (any channel)
 *   target_comm_new       : ncclCommInitRank on the calling thread's current HIP device (collective over all ranks)
 *   ..._gather_pose_begin : enqueue.  counts [world] = rows per rank (counts[rank] == target_manager_size);
 *                           recv_dev (root only) [sum(counts)][7] doubles, rank r's rows at row sum(counts[:r]), batch
 *                           order then slot order within a rank.  Returns immediately.
 *   ..._gather_pose_wait  : block the host until the last gather has finished; device_ms (may be NULL) = its duration
 * RCCL is looked up at run time (the copy already in the process, else librccl.so.1). */
typedef void target_comm_c;
int target_comm_unique_id(char* out128);
target_comm_c* target_comm_new(const char* id128, int rank, int world);
void target_comm_delete(target_comm_c* comm);
int target_manager_gather_pose_begin(target_manager_c* self, target_comm_c* comm, int root, const long* counts, double* recv_dev);
int target_manager_gather_pose_wait(target_comm_c* comm, float* device_ms);
/* the same with a deadline (the done event is polled with hipEventQuery): 0 finished, 1 still in flight after timeout_s
 * seconds (a peer that never posted its send / recv; nothing is cancelled), < 0 error */
int target_manager_gather_pose_wait_for(target_comm_c* comm, double timeout_s, float* device_ms);

/* ---- measurement ingest: the ROS node's mailbox / has-measurement / expiry policy --------------- */
/* Transport-agnostic restatement of class Measurement (target_manager_ros.hpp:74-134) and
 * RosTargetManager::update (src/target_manager_ros.cpp:41-92).  The caller pushes (id | frame name,
 * stamp, pose); one tick = create the targets seen for the first time, predict+update those whose
 * mailbox holds a new measurement, predict the others, erase those whose last measurement is older
 * than the expiration time; as one batched init + one batched step.
 * Q == NULL: new targets use the manager's default model (then type, R, P0 are ignored). */
typedef void target_ingest_c;
target_ingest_c* target_ingest_new(target_manager_c* manager, int type, const double* Q, const double* R, const double* P0);
void target_ingest_delete(target_ingest_c* ingest);
void target_ingest_set_expiration_time(target_ingest_c* ingest, double seconds);   /* setExpirationTime, :99-103 */
void target_ingest_set_token_name(target_ingest_c* ingest, const char* token);      /* setTargetTokenName, :94-97 */
int target_ingest_push(target_ingest_c* ingest, unsigned int id, double stamp, const double* pose);
/* 1 taken, 0 frame name without the token, -1 token present but not "<name>_<id>" (the reference then
 * drops the rest of the message, target_manager_ros.cpp:34-35) */
int target_ingest_push_named(target_ingest_c* ingest, const char* child_frame_id, double stamp, const double* pose);
/* one node tick at wall time `now`; ids_out / poses_out ([capacity], [capacity][7]) receive the live
 * targets in ascending id order with their filtered poses; returns their number */
long target_ingest_tick(target_ingest_c* ingest, double dt, double now, unsigned int* ids_out, double* poses_out, long capacity);

#ifdef __cplusplus
}
#endif
#endif
