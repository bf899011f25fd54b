// target_manager_c.cpp -- extern "C" boundary over te::TargetManager.
// The first ten functions are the reference's C wrapper (src/target_manager_c.cpp:15-76,
// declared in include/target_estimation/target_manager_c.h:28-37); the rest is the batched
// extension declared in include/target_estimation_amd/target_batch_c.h.
#include <cstdio>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/target_estimation_amd/target_batch_c.h"
#include "intersection_solver.hpp"
#include "measurement_ingest.hpp"
#include "pose_gather.hpp"
#include "stream_gen.hpp"
#include "target_manager.hpp"

using te::Batch;
using te::TargetManager;

namespace {
thread_local std::string g_last_error;

void set_error(const char* where, const char* what) {
  g_last_error = std::string(where) + ": " + what;
  std::fprintf(stderr, "[target_estimation_amd] %s\n", g_last_error.c_str());
}

// run f(); map the reference's thrown `const char*` / std::exception to an error code
template <class F>
int guarded(const char* where, F&& f) {
  try {
    f();
    return 0;
  } catch (const char* msg) {
    set_error(where, msg);
  } catch (const std::exception& e) {
    set_error(where, e.what());
  } catch (...) {
    set_error(where, "unknown exception");
  }
  return -1;
}

// f()'s value, or `fallback` (with the error recorded) if it throws
template <class R, class F>
R guarded_value(const char* where, R fallback, F&& f) {
  R out = fallback;
  guarded(where, [&] { out = f(); });
  return out;
}

// a NULL handle is reported like any other error (the reference dereferences it)
inline TargetManager* M(const target_manager_c* self) {
  if (!self) throw std::invalid_argument("NULL manager handle");
  return (TargetManager*)self;
}
inline Batch* B(target_batch_c* b) {
  if (!b) throw std::invalid_argument("NULL batch handle");
  return (Batch*)b;
}
// Calls through a batch handle take the owning manager's mutex (the same one every TargetManager method takes), so a
// thread on the ten-symbol ABI and a thread driving a batch handle are serialised; Batch itself is not locked.
struct BatchLock {
  std::unique_lock<std::mutex> l;
  explicit BatchLock(Batch* b) { if (b->owner_lock()) l = std::unique_lock<std::mutex>(*b->owner_lock()); }
};
inline te::MeasurementIngest* I(target_ingest_c* i) {
  if (!i) throw std::invalid_argument("NULL ingest handle");
  return (te::MeasurementIngest*)i;
}
// the pose stream of a ..._poses call (target_pose_stream_c; NULL or a NULL pose_dev: none)
te::PoseStream pose_stream(const target_pose_stream_c* p) {
  te::PoseStream q;
  if (p && p->pose_dev) { q.dev = p->pose_dev; q.ld = p->ld; q.tick_stride = p->tick_stride; q.ring = p->ring_ticks; }
  return q;
}
// the innovation stream of a ..._innov call (target_innov_stream_c; NULL or a NULL nis_dev: none)
te::InnovStream innov_stream(const target_innov_stream_c* p) {
  te::InnovStream q;
  if (p && p->nis_dev) {
    q.nis = p->nis_dev; q.innov = p->innov_dev; q.ld = p->ld; q.nis_tick_stride = p->nis_tick_stride;
    q.innov_tick_stride = p->innov_tick_stride; q.ring = p->ring_ticks;
  }
  return q;
}
// the same with the gate of a ..._gated call: nis_max 0 = none, > 0 (+inf included) = gated; anything else, or a gate without a
// NIS row, is refused before a handle is looked at
te::InnovStream gated_stream(const target_innov_stream_c* p, double nis_max) {
  if (!(nis_max >= 0.0)) throw std::invalid_argument("gate: nis_max must be 0 (no gate) or positive, got " + std::to_string(nis_max));
  te::InnovStream q = innov_stream(p);
  if (nis_max > 0.0 && !q.nis) throw std::invalid_argument("gate: nis_max > 0 needs an innovation stream with a NIS row (nis_dev): it reports the decisions");
  q.gate = nis_max > 0.0 ? nis_max : 0.0;
  return q;
}
// the same with the re-acquisition policy of a ..._reacquire call (NULL, or max_rejects < 0 in a per-batch array: none)
te::InnovStream reacquire_stream(const target_innov_stream_c* p, double nis_max, const target_reacquire_c* r, bool per_batch) {
  te::InnovStream q = gated_stream(p, nis_max);
  if (!r || (per_batch && r->max_rejects < 0)) return q;
  if (r->max_rejects < 0 || r->max_rejects > 127) throw std::invalid_argument("re-acquisition: max_rejects must be 0..127, got " + std::to_string(r->max_rejects));
  if (!q.gated()) throw std::invalid_argument("re-acquisition: a policy needs the gate (nis_max > 0): it counts the gate's rejections");
  q.reacq.on = true; q.reacq.k = r->max_rejects; q.reacq.event = r->event_dev;
  if (r->event_dev) {
    if (r->ld <= 0 || r->tick_stride < 0 || (r->tick_stride > 0 && r->tick_stride < r->ld) || r->ring_ticks < 0)
      throw std::invalid_argument("re-acquisition: event rows need ld > 0, tick_stride 0 or >= ld, ring_ticks >= 0");
    q.reacq.ld = r->ld; q.reacq.tick_stride = r->tick_stride; q.reacq.ring = r->ring_ticks;
  }
  return q;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------- the reference's ten symbols
target_manager_c* target_manager_new(const char* file) {
  return target_manager_new_ex(file, TARGET_DTYPE_F64, 0);
}

void target_manager_init(const target_manager_c* self, const unsigned int id, const double dt0, double p0[], const double t0) {
  guarded("target_manager_init", [&] { M(self)->init(id, dt0, t0, p0); });
}

void target_manager_update_meas(const target_manager_c* self, const unsigned int id, const double dt, double meas[]) {
  guarded("target_manager_update_meas", [&] { M(self)->update(id, dt, meas); });
}

void target_manager_update(const target_manager_c* self, const unsigned int id, const double dt) {
  guarded("target_manager_update", [&] { M(self)->update(id, dt); });
}

bool target_manager_get_est_pose(const target_manager_c* self, const unsigned int id, double pose[]) {
  bool res = false;
  guarded("target_manager_get_est_pose", [&] { res = M(self)->getTargetPose(id, pose); });
  return res;
}

bool target_manager_get_est_twist(const target_manager_c* self, const unsigned int id, double twist[]) {
  bool res = false;
  guarded("target_manager_get_est_twist", [&] { res = M(self)->getTargetTwist(id, twist); });
  return res;
}

bool target_manager_get_est_acceleration(const target_manager_c* self, const unsigned int id, double acceleration[]) {
  bool res = false;
  guarded("target_manager_get_est_acceleration", [&] { res = M(self)->getTargetAcceleration(id, acceleration); });
  return res;
}

int target_manager_get_n_measurements(const target_manager_c* self, const unsigned int id) {
  int n = 0;
  guarded("target_manager_get_n_measurements", [&] { n = (int)M(self)->getNumberMeasurements(id); });
  return n;
}

void target_manager_log(const target_manager_c* self) {
  guarded("target_manager_log", [&] { M(self)->log(); });
}

void target_manager_delete(target_manager_c* self) {
  if (self) guarded("target_manager_delete", [&] { delete M(self); });
}

// ---------------------------------------------------------------- batched extension
target_manager_c* target_manager_new_ex(const char* file, int dtype, int lanes_per_target) {
  TargetManager* m = nullptr;
  guarded("target_manager_new", [&] {
    m = file ? new TargetManager(std::string(file), dtype, lanes_per_target) : new TargetManager(dtype, lanes_per_target);
  });
  return (target_manager_c*)m;
}

int target_manager_set_stream(target_manager_c* self, void* hip_stream) {
  return guarded("target_manager_set_stream", [&] { M(self)->setStream((hipStream_t)hip_stream); });
}

int target_manager_set_log_directory(target_manager_c* self, const char* dir) {
  return guarded("target_manager_set_log_directory", [&] { M(self)->setLogDirectory(dir ? dir : ""); });
}

int target_manager_synchronize(target_manager_c* self) {
  return guarded("target_manager_synchronize", [&] { M(self)->synchronize(); });
}

const char* target_manager_last_error(void) { return g_last_error.c_str(); }

int target_manager_init_typed(target_manager_c* self, int type, unsigned int id, double dt0, double t0, const double* Q,
                              const double* R, const double* P0, const double* p0, const double* v0, const double* a0) {
  return guarded("target_manager_init_typed", [&] {
    M(self)->init((TargetManager::target_t)type, id, dt0, t0, Q, R, P0, p0, v0, a0);
  });
}

long target_manager_init_batch(target_manager_c* self, const unsigned int* ids, long n, double dt0, double t0,
                               const double* p0, const double* v0, const double* a0) {
  long k = -1;
  guarded("target_manager_init_batch", [&] { k = M(self)->initBatch(ids, n, dt0, t0, p0, v0, a0); });
  return k;
}

long target_manager_init_batch_typed(target_manager_c* self, int type, const unsigned int* ids, long n, double dt0,
                                     double t0, const double* Q, const double* R, const double* P0, int per_target_P0,
                                     const double* p0, const double* v0, const double* a0) {
  long k = -1;
  guarded("target_manager_init_batch_typed", [&] {
    k = M(self)->initBatch((TargetManager::target_t)type, ids, n, dt0, t0, Q, R, P0, per_target_P0 != 0, p0, v0, a0);
  });
  return k;
}

long target_manager_init_batch_classes(target_manager_c* self, int type, const unsigned int* ids, long n, double dt0, double t0,
                                       long n_classes, const double* Q, const double* R, const double* P0,
                                       const unsigned int* class_of, const double* p0, const double* v0, const double* a0) {
  long k = -1;
  guarded("target_manager_init_batch_classes", [&] {
    if (!ids || !Q || !R || !P0 || !class_of || !p0) throw std::invalid_argument("NULL argument");
    k = M(self)->initBatchClasses((TargetManager::target_t)type, ids, n, dt0, t0, n_classes, Q, R, P0, class_of, p0, v0, a0);
  });
  return k;
}

int target_batch_num_classes(target_batch_c* b) {
  return guarded_value<int>("target_batch_num_classes", -1, [&]() -> int { return B(b)->n_classes(); });
}

int target_manager_erase(target_manager_c* self, unsigned int id) {
  int r = -1;
  guarded("target_manager_erase", [&] { r = M(self)->erase(id) ? 1 : 0; });
  return r;
}

long target_manager_erase_batch(target_manager_c* self, const unsigned int* ids, long n) {
  long k = -1;
  guarded("target_manager_erase_batch", [&] { k = M(self)->eraseBatch(ids, n); });
  return k;
}

long target_manager_size(target_manager_c* self) {
  long n = -1;
  guarded("target_manager_size", [&] { n = (long)M(self)->size(); });
  return n;
}

long target_manager_get_available_targets(target_manager_c* self, unsigned int* ids_out, long capacity) {
  long n = -1;
  guarded("target_manager_get_available_targets", [&] {
    auto ids = M(self)->getAvailableTargets();
    n = (long)ids.size();
    for (long i = 0; i < n && i < capacity; ++i) ids_out[i] = ids[(size_t)i];
  });
  return n;
}

long target_manager_update_meas_batch(target_manager_c* self, const unsigned int* ids, long n, double dt,
                                      const double* meas, const unsigned char* has_meas) {
  long k = -1;
  guarded("target_manager_update_meas_batch", [&] { k = M(self)->updateBatch(ids, n, dt, meas, has_meas); });
  return k;
}

int target_manager_update_all(target_manager_c* self, double dt) {
  return guarded("target_manager_update_all", [&] { M(self)->update(dt); });
}

long target_manager_get_est_batch(target_manager_c* self, const unsigned int* ids, long n, double* pose, double* twist,
                                  double* acceleration, unsigned char* found) {
  long k = -1;
  guarded("target_manager_get_est_batch", [&] { k = M(self)->getPoseBatch(ids, n, pose, twist, acceleration, found); });
  return k;
}

long target_manager_get_est_at_batch(target_manager_c* self, const unsigned int* ids, long n, double t1, double* pose,
                                     double* twist, double* acceleration, unsigned char* found) {
  long k = -1;
  guarded("target_manager_get_est_at_batch", [&] {
    k = M(self)->getPoseBatch(ids, n, pose, twist, acceleration, found, true, t1);
  });
  return k;
}

long target_manager_get_state_batch(target_manager_c* self, const unsigned int* ids, long n, double* x, double* P) {
  long k = -1;
  guarded("target_manager_get_state_batch", [&] { k = M(self)->getStateBatch(ids, n, x, P); });
  return k;
}

int target_manager_get_time(target_manager_c* self, unsigned int id, double* t) {
  int r = -1;
  guarded("target_manager_get_time", [&] { r = M(self)->getTargetTime(id, *t) ? 0 : -2; });
  return r;
}

double target_manager_get_intersection_time_with_sphere(target_manager_c* self, unsigned int id, double t1,
                                                         const double* origin, double radius) {
  double d = -1;
  guarded("target_manager_get_intersection_time_with_sphere", [&] {
    d = M(self)->getIntersectionTimeWithSphere(id, t1, origin, radius);
  });
  return d;
}

bool target_manager_get_intersection_pose_with_sphere(target_manager_c* self, unsigned int id, double t1,
                                                      const double* origin, double radius, double* pose,
                                                      double* delta) {
  bool r = false;
  guarded("target_manager_get_intersection_pose_with_sphere", [&] {
    r = M(self)->getIntersectionPoseWithSphere(id, t1, origin, radius, pose, delta);
  });
  return r;
}

long target_manager_intersect_sphere_batch(target_manager_c* self, const unsigned int* ids, long n, double t1,
                                           const double* origin, double radius, double* delta, double* pose,
                                           unsigned char* found) {
  long k = -1;
  guarded("target_manager_intersect_sphere_batch", [&] {
    k = M(self)->intersectBatch(ids, n, t1, origin, radius, delta, pose, found);
  });
  return k;
}

long target_manager_intersect_sphere_converged_batch(target_manager_c* self, const unsigned int* ids, long n, double t1,
                                                     double pos_th, double ang_th, const double* origin, double radius,
                                                     int filters_length, double* delta, double* pose,
                                                     unsigned char* converged, unsigned char* found, double* filtered_errors) {
  long k = -1;
  guarded("target_manager_intersect_sphere_converged_batch", [&] {
    M(self)->setIntersectionFiltersLength(filters_length > 0 ? filters_length : 250);
    k = M(self)->intersectGatedBatch(ids, n, t1, pos_th, ang_th, origin, radius, delta, pose, converged, found, filtered_errors);
  });
  return k;
}

int target_batch_intersect_sphere_converged_dev(target_batch_c* b, double t1, double pos_th, double ang_th,
                                                const double* origin, double radius, int filters_length,
                                                double* delta_dev, double* pose_dev, unsigned char* converged_dev) {
  return guarded("target_batch_intersect_sphere_converged_dev", [&] { BatchLock lk(B(b));
    B(b)->intersect_gated_dev(t1, origin, radius, pos_th, ang_th, filters_length > 0 ? filters_length : 250, delta_dev,
                              pose_dev, converged_dev);
  });
}

int target_batch_gate_update_dev(target_batch_c* b, const double* delta_dev, const double* pose_dev, double pos_th, double ang_th,
                                 int filters_length, unsigned char* converged_dev, double* filtered_dev, double* variance_dev) {
  return guarded("target_batch_gate_update_dev", [&] { BatchLock lk(B(b));
    if (!delta_dev || !pose_dev || !converged_dev) throw std::invalid_argument("delta, pose and converged are required");
    B(b)->gate_update_dev(delta_dev, pose_dev, pos_th, ang_th, filters_length > 0 ? filters_length : 250, converged_dev, filtered_dev,
                          variance_dev);
  });
}

// ---- the k soonest crossings (select_soonest.hpp).  The host forms write their arrays only after the call has succeeded.
int target_batch_select_soonest_dev(target_batch_c* b, const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev,
                                    double delta_lo, double delta_hi, long k, int* slot_out_dev, double* delta_out_dev,
                                    double* pose_out_dev, int* count_out_dev) {
  return guarded_value<int>("target_batch_select_soonest_dev", -1, [&]() -> int { BatchLock lk(B(b));
    B(b)->select_soonest_dev(delta_dev, pose_dev, ok_dev, delta_lo, delta_hi, k, slot_out_dev, delta_out_dev, pose_out_dev, count_out_dev);
    return 0;
  });
}

long target_batch_select_soonest(target_batch_c* b, const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev,
                                 double delta_lo, double delta_hi, long k, unsigned int* ids_out, int* slots_out, double* delta_out,
                                 double* pose_out) {
  return guarded_value<long>("target_batch_select_soonest", -1L, [&]() -> long { BatchLock lk(B(b));
    te::check_soonest_args(k, delta_lo, delta_hi, delta_dev != nullptr, pose_dev != nullptr, pose_out != nullptr,
                           ids_out != nullptr && slots_out != nullptr && delta_out != nullptr);
    std::vector<te::SoonestRow> rows((size_t)k);
    const long count = B(b)->select_soonest(delta_dev, pose_dev, ok_dev, delta_lo, delta_hi, k, pose_out != nullptr, rows.data());
    for (long i = 0; i < k; ++i) {
      const te::SoonestRow& r = rows[(size_t)i];
      ids_out[i] = i < count ? B(b)->slot_id(r.slot) : ~0u;
      slots_out[i] = r.slot; delta_out[i] = r.delta;
      if (pose_out) for (int c = 0; c < 7; ++c) pose_out[i * 7 + c] = r.pose[c];
    }
    return count;
  });
}

static std::vector<te::SoonestSpec> soonest_specs(const target_batch_sequence_c* per_batch, long n_batches, const unsigned char* const* ok) {
  if (n_batches < 0 || (n_batches > 0 && !per_batch)) throw std::invalid_argument("target_estimation_amd: select_soonest: one description per batch is needed");
  std::vector<te::SoonestSpec> specs((size_t)n_batches);
  for (long i = 0; i < n_batches; ++i) specs[(size_t)i] = te::SoonestSpec{per_batch[i].delta_dev, per_batch[i].pose_dev, ok ? ok[i] : nullptr};
  return specs;
}

long target_manager_select_soonest(target_manager_c* m, const target_batch_sequence_c* per_batch, long n_batches,
                                   const unsigned char* const* ok_dev_per_batch, double delta_lo, double delta_hi, long k,
                                   unsigned int* ids_out, int* batch_out, int* slots_out, double* delta_out, double* pose_out) {
  return guarded_value<long>("target_manager_select_soonest", -1L, [&]() -> long {
    TargetManager* mgr = M(m);
    te::check_soonest_args(k, delta_lo, delta_hi, true, pose_out != nullptr, pose_out != nullptr,
                           ids_out != nullptr && batch_out != nullptr && slots_out != nullptr && delta_out != nullptr);
    const std::vector<te::SoonestSpec> specs = soonest_specs(per_batch, n_batches, ok_dev_per_batch);
    std::vector<te::SoonestRow> rows((size_t)k);
    std::vector<unsigned> ids((size_t)k);
    const long count = mgr->selectSoonest(specs.data(), n_batches, delta_lo, delta_hi, k, pose_out != nullptr, rows.data(), ids.data());
    for (long i = 0; i < k; ++i) {
      const te::SoonestRow& r = rows[(size_t)i];
      ids_out[i] = ids[(size_t)i]; batch_out[i] = r.batch; slots_out[i] = r.slot; delta_out[i] = r.delta;
      if (pose_out) for (int c = 0; c < 7; ++c) pose_out[i * 7 + c] = r.pose[c];
    }
    return count;
  });
}

int target_manager_select_soonest_dev(target_manager_c* m, const target_batch_sequence_c* per_batch, long n_batches,
                                      const unsigned char* const* ok_dev_per_batch, double delta_lo, double delta_hi, long k,
                                      int* batch_out_dev, int* slot_out_dev, double* delta_out_dev, double* pose_out_dev,
                                      int* count_out_dev) {
  return guarded_value<int>("target_manager_select_soonest_dev", -1, [&]() -> int {
    TargetManager* mgr = M(m);
    const std::vector<te::SoonestSpec> specs = soonest_specs(per_batch, n_batches, ok_dev_per_batch);
    mgr->selectSoonestDev(specs.data(), n_batches, delta_lo, delta_hi, k, te::SoonestOut{batch_out_dev, slot_out_dev, delta_out_dev, pose_out_dev, count_out_dev});
    return 0;
  });
}

// ---- position covariance and time spread at a crossing (crossing_cov.hpp).  What does not depend on the handle is refused before
// the handle is looked at.
int target_batch_crossing_cov_dev(target_batch_c* b, double t1, const double* origin, double radius, const double* delta_dev,
                                  const int* slots_dev, long n, double sigma_r_max, double sigma_t_max, double* cov_out_dev,
                                  double* sigma_out_dev, unsigned char* ok_out_dev) {
  return guarded("target_batch_crossing_cov_dev", [&] {
    te::check_crossing_cov_args(delta_dev != nullptr, origin != nullptr, radius, cov_out_dev != nullptr, sigma_out_dev != nullptr,
                                ok_out_dev != nullptr, sigma_r_max, sigma_t_max, slots_dev != nullptr, n, n);
    BatchLock lk(B(b));
    B(b)->crossing_cov_dev(t1, origin, radius, delta_dev, slots_dev, n, sigma_r_max, sigma_t_max, cov_out_dev, sigma_out_dev, ok_out_dev);
  });
}

int target_manager_crossing_cov_dev(target_manager_c* m, double t1, const double* origin, double radius, const int* batch_dev,
                                    const int* slots_dev, const double* delta_dev, long n, double sigma_r_max, double sigma_t_max,
                                    double* cov_out_dev, double* sigma_out_dev, unsigned char* ok_out_dev) {
  return guarded("target_manager_crossing_cov_dev", [&] {
    te::check_crossing_cov_args(delta_dev != nullptr, origin != nullptr, radius, cov_out_dev != nullptr, sigma_out_dev != nullptr,
                                ok_out_dev != nullptr, sigma_r_max, sigma_t_max, true, n, 0);
    if (!batch_dev || !slots_dev) throw std::invalid_argument("target_estimation_amd: crossing_cov: the batch and slot lists are required");
    M(m)->crossingCovDev(t1, origin, radius, batch_dev, slots_dev, delta_dev, n, sigma_r_max, sigma_t_max, cov_out_dev, sigma_out_dev, ok_out_dev);
  });
}

long target_manager_crossing_cov_batch(target_manager_c* m, const unsigned int* ids, long n, double t1, const double* origin, double radius,
                                       const double* delta_host, double sigma_r_max, double sigma_t_max, double* cov_out,
                                       double* sigma_out, unsigned char* ok_out) {
  return guarded_value<long>("target_manager_crossing_cov_batch", -1L, [&]() -> long {
    te::check_crossing_cov_args(delta_host != nullptr, origin != nullptr, radius, cov_out != nullptr, sigma_out != nullptr, ok_out != nullptr,
                                sigma_r_max, sigma_t_max, false, n, n);
    return M(m)->crossingCovBatch(ids, n, t1, origin, radius, delta_host, sigma_r_max, sigma_t_max, cov_out, sigma_out, ok_out);
  });
}

// ---- association of unlabelled detections (associate.hpp).  What does not depend on the handle is refused before the handle is
// looked at; the host forms write their arrays only after the call has succeeded.
static TargetManager* assoc_manager(const target_manager_c* m) { return M(m); }   // (the ABI names the detection count M)
static std::vector<te::AssocSlotOut> assoc_outs(const target_assoc_out_c* per_batch, long n_batches) {
  if (n_batches < 0 || (n_batches > 0 && !per_batch)) throw std::invalid_argument("target_estimation_amd: associate: one output description per batch is needed");
  std::vector<te::AssocSlotOut> outs((size_t)n_batches);
  for (long i = 0; i < n_batches; ++i) {
    te::AssocSlotOut& o = outs[(size_t)i];
    o.meas = per_batch[i].meas_out_dev; o.ld = per_batch[i].ld; o.has_meas = per_batch[i].has_meas_out_dev;
    o.det_of_slot = per_batch[i].det_of_slot_dev; o.d2_of_slot = per_batch[i].d2_of_slot_dev;
  }
  return outs;
}

int target_batch_associate_dev(target_batch_c* b, double dt, const double* det_dev, long M, double gate, int rounds, void* meas_out_dev,
                               long ld, unsigned char* has_meas_out_dev, int* det_of_slot_dev, double* d2_of_slot_dev,
                               int* slot_of_det_dev, double* d2_of_det_dev, int* info_dev) {
  return guarded("target_batch_associate_dev", [&] {
    te::check_assoc_args(dt, det_dev != nullptr, M, gate, rounds, meas_out_dev != nullptr && has_meas_out_dev != nullptr && info_dev != nullptr, 0, 0);
    BatchLock lk(B(b));
    te::AssocSlotOut out;
    out.meas = meas_out_dev; out.ld = ld; out.has_meas = has_meas_out_dev; out.det_of_slot = det_of_slot_dev; out.d2_of_slot = d2_of_slot_dev;
    B(b)->associate_dev(dt, det_dev, M, gate, rounds, out, slot_of_det_dev, d2_of_det_dev, info_dev);
  });
}

long target_batch_associate(target_batch_c* b, double dt, const double* det_host, long M, double gate, int rounds, void* meas_out_dev,
                            long ld, unsigned char* has_meas_out_dev, unsigned int* ids_of_det_out, int* slot_of_det_out,
                            double* d2_of_det_out, long* unmatched_out, long* n_unmatched_out, int* info_out) {
  return guarded_value<long>("target_batch_associate", -1L, [&]() -> long {
    te::check_assoc_args(dt, det_host != nullptr, M, gate, rounds, true, 0, 0);
    BatchLock lk(B(b));
    te::AssocSlotOut out;
    out.meas = meas_out_dev; out.ld = ld; out.has_meas = has_meas_out_dev;
    return B(b)->associate(dt, det_host, M, gate, rounds, out, ids_of_det_out, slot_of_det_out, d2_of_det_out, unmatched_out, n_unmatched_out, info_out);
  });
}

int target_manager_associate_dev(target_manager_c* m, double dt, const double* det_dev, long M, double gate, int rounds,
                                 const target_assoc_out_c* per_batch, long n_batches, int* slot_of_det_dev, int* batch_of_det_dev,
                                 double* d2_of_det_dev, int* info_dev) {
  return guarded("target_manager_associate_dev", [&] {
    te::check_assoc_args(dt, det_dev != nullptr, M, gate, rounds, info_dev != nullptr, 0, 0);
    TargetManager* mgr = assoc_manager(m);
    const std::vector<te::AssocSlotOut> outs = assoc_outs(per_batch, n_batches);
    mgr->associateDev(dt, det_dev, M, gate, rounds, outs.data(), n_batches, slot_of_det_dev, batch_of_det_dev, d2_of_det_dev, info_dev);
  });
}

long target_manager_associate(target_manager_c* m, double dt, const double* det_host, long M, double gate, int rounds,
                              const target_assoc_out_c* per_batch, long n_batches, unsigned int* ids_of_det_out, int* batch_of_det_out,
                              int* slot_of_det_out, double* d2_of_det_out, long* unmatched_out, long* n_unmatched_out, int* info_out) {
  return guarded_value<long>("target_manager_associate", -1L, [&]() -> long {
    te::check_assoc_args(dt, det_host != nullptr, M, gate, rounds, true, 0, 0);
    TargetManager* mgr = assoc_manager(m);
    const std::vector<te::AssocSlotOut> outs = assoc_outs(per_batch, n_batches);
    return mgr->associate(dt, det_host, M, gate, rounds, per_batch ? outs.data() : nullptr, n_batches, ids_of_det_out, batch_of_det_out,
                          slot_of_det_out, d2_of_det_out, unmatched_out, n_unmatched_out, info_out);
  });
}

// ---- the grid form (associate_grid.hpp): the same entry points with grid_cell set
int target_batch_associate_grid_dev(target_batch_c* b, double dt, const double* det_dev, long M, double gate, int rounds, double cell,
                                    void* meas_out_dev, long ld, unsigned char* has_meas_out_dev, int* det_of_slot_dev,
                                    double* d2_of_slot_dev, int* slot_of_det_dev, double* d2_of_det_dev, int* info_dev) {
  return guarded("target_batch_associate_grid_dev", [&] {
    te::check_assoc_grid_args(dt, det_dev != nullptr, M, gate, rounds, cell, meas_out_dev != nullptr && has_meas_out_dev != nullptr && info_dev != nullptr, 0, 0);
    BatchLock lk(B(b));
    te::AssocSlotOut out;
    out.meas = meas_out_dev; out.ld = ld; out.has_meas = has_meas_out_dev; out.det_of_slot = det_of_slot_dev; out.d2_of_slot = d2_of_slot_dev;
    B(b)->associate_dev(dt, det_dev, M, gate, rounds, out, slot_of_det_dev, d2_of_det_dev, info_dev, cell);
  });
}

long target_batch_associate_grid(target_batch_c* b, double dt, const double* det_host, long M, double gate, int rounds, double cell,
                                 void* meas_out_dev, long ld, unsigned char* has_meas_out_dev, unsigned int* ids_of_det_out,
                                 int* slot_of_det_out, double* d2_of_det_out, long* unmatched_out, long* n_unmatched_out, int* info_out) {
  return guarded_value<long>("target_batch_associate_grid", -1L, [&]() -> long {
    te::check_assoc_grid_args(dt, det_host != nullptr, M, gate, rounds, cell, true, 0, 0);
    BatchLock lk(B(b));
    te::AssocSlotOut out;
    out.meas = meas_out_dev; out.ld = ld; out.has_meas = has_meas_out_dev;
    return B(b)->associate(dt, det_host, M, gate, rounds, out, ids_of_det_out, slot_of_det_out, d2_of_det_out, unmatched_out, n_unmatched_out, info_out,
                           cell);
  });
}

int target_manager_associate_grid_dev(target_manager_c* m, double dt, const double* det_dev, long M, double gate, int rounds, double cell,
                                      const target_assoc_out_c* per_batch, long n_batches, int* slot_of_det_dev, int* batch_of_det_dev,
                                      double* d2_of_det_dev, int* info_dev) {
  return guarded("target_manager_associate_grid_dev", [&] {
    te::check_assoc_grid_args(dt, det_dev != nullptr, M, gate, rounds, cell, info_dev != nullptr, 0, 0);
    TargetManager* mgr = assoc_manager(m);
    const std::vector<te::AssocSlotOut> outs = assoc_outs(per_batch, n_batches);
    mgr->associateDev(dt, det_dev, M, gate, rounds, outs.data(), n_batches, slot_of_det_dev, batch_of_det_dev, d2_of_det_dev, info_dev, cell);
  });
}

long target_manager_associate_grid(target_manager_c* m, double dt, const double* det_host, long M, double gate, int rounds, double cell,
                                   const target_assoc_out_c* per_batch, long n_batches, unsigned int* ids_of_det_out,
                                   int* batch_of_det_out, int* slot_of_det_out, double* d2_of_det_out, long* unmatched_out,
                                   long* n_unmatched_out, int* info_out) {
  return guarded_value<long>("target_manager_associate_grid", -1L, [&]() -> long {
    te::check_assoc_grid_args(dt, det_host != nullptr, M, gate, rounds, cell, true, 0, 0);
    TargetManager* mgr = assoc_manager(m);
    const std::vector<te::AssocSlotOut> outs = assoc_outs(per_batch, n_batches);
    return mgr->associate(dt, det_host, M, gate, rounds, per_batch ? outs.data() : nullptr, n_batches, ids_of_det_out, batch_of_det_out,
                          slot_of_det_out, d2_of_det_out, unmatched_out, n_unmatched_out, info_out, cell);
  });
}

int target_batch_intersect_sphere_dev(target_batch_c* b, double t1, const double* origin, double radius,
                                      double* delta_dev, double* pose_dev) {
  return guarded("target_batch_intersect_sphere_dev", [&] { BatchLock lk(B(b)); B(b)->intersect_dev(t1, origin, radius, delta_dev, pose_dev); });
}

int target_manager_num_batches(target_manager_c* self) {
  return guarded_value<int>("target_manager_num_batches", -1, [&]() -> int { return M(self)->numBatches(); });
}

target_batch_c* target_manager_get_batch(target_manager_c* self, int index) {
  return guarded_value<target_batch_c*>("target_manager_get_batch", nullptr, [&]() -> target_batch_c* {
    if (index < 0 || index >= M(self)->numBatches()) return nullptr;
    return (target_batch_c*)M(self)->batch(index);
  });
}

target_batch_c* target_manager_get_batch_of_type(target_manager_c* self, int type) {
  return guarded_value<target_batch_c*>("target_manager_get_batch_of_type", nullptr,
                                        [&]() -> target_batch_c* { return (target_batch_c*)M(self)->batchOfType(type); });
}

long target_batch_size(target_batch_c* b) {
  return guarded_value<long>("target_batch_size", -1, [&]() -> long { return B(b)->size(); });
}
int target_batch_type(target_batch_c* b) {
  return guarded_value<int>("target_batch_type", -1, [&]() -> int { return B(b)->type(); });
}
int target_batch_dtype(target_batch_c* b) {
  return guarded_value<int>("target_batch_dtype", -1, [&]() -> int { return B(b)->dtype(); });
}
int target_batch_state_dim(target_batch_c* b) {
  return guarded_value<int>("target_batch_state_dim", -1, [&]() -> int { return B(b)->n_state(); });
}
int target_batch_meas_dim(target_batch_c* b) {
  return guarded_value<int>("target_batch_meas_dim", -1, [&]() -> int { return B(b)->n_meas(); });
}
int target_batch_lanes_per_target(target_batch_c* b) {
  return guarded_value<int>("target_batch_lanes_per_target", -1, [&]() -> int { return B(b)->layout().g; });
}
int target_batch_is_symmetric_packed(target_batch_c* b) {
  return guarded_value<int>("target_batch_is_symmetric_packed", -1, [&]() -> int { return B(b)->layout().layout == te::LAYOUT_PACKED; });
}
int target_batch_layout(target_batch_c* b) {
  return guarded_value<int>("target_batch_layout", -1, [&]() -> int { return B(b)->layout().layout; });
}
int target_batch_shared_axes(target_batch_c* b) {
  return guarded_value<int>("target_batch_shared_axes", -1, [&]() -> int { return B(b)->shared_axes() ? 1 : 0; });
}
long target_batch_uniform_tiles(target_batch_c* b) {
  return guarded_value<long>("target_batch_uniform_tiles", -1, [&]() -> long { BatchLock lk(B(b)); return B(b)->uniform_tiles(); });
}
int target_batch_record_words(target_batch_c* b) {
  return guarded_value<int>("target_batch_record_words", -1, [&]() -> int { return B(b)->layout().record_words; });
}
long target_batch_algorithmic_bytes(target_batch_c* b) {
  return guarded_value<long>("target_batch_algorithmic_bytes", -1, [&]() -> long { BatchLock lk(B(b)); return B(b)->algorithmic_bytes_per_cycle(); });   // (reads the tile flags back: batch_store.cpp)
}
double target_batch_resident_bytes_per_target(target_batch_c* b) {
  return guarded_value<double>("target_batch_resident_bytes_per_target", -1.0,
                               [&]() -> double { return (double)B(b)->layout().tile_bytes / (double)B(b)->layout().tpw; });
}

long target_batch_slot_ids(target_batch_c* b, unsigned int* ids_out, long capacity) {
  return guarded_value<long>("target_batch_slot_ids", -1, [&]() -> long {
    BatchLock lk(B(b));
    const auto& ids = B(b)->slot_ids();
    const long n = (long)ids.size();
    for (long i = 0; i < n && i < capacity; ++i) ids_out[i] = ids[(size_t)i];
    return n;
  });
}

int target_batch_step(target_batch_c* b, double dt, const void* meas_dev, long ld, const unsigned char* has_meas_dev) {
  return guarded("target_batch_step", [&] { BatchLock lk(B(b)); B(b)->step_dense(dt, meas_dev, ld, has_meas_dev); });
}

int target_batch_step_host(target_batch_c* b, double dt, const void* meas_soa_host, long ld_host, const unsigned char* has_meas_host) {
  return guarded("target_batch_step_host", [&] { BatchLock lk(B(b)); B(b)->step_dense_host_soa(dt, meas_soa_host, ld_host, has_meas_host); });
}

static te::DtSchedule dt_schedule(long n_ticks, const double* dt_host) {
  if (n_ticks > 0 && !dt_host) throw std::invalid_argument("dt_host must not be NULL");
  return n_ticks > 0 ? te::DtSchedule(dt_host, n_ticks) : te::DtSchedule();
}

// The target_batch_step_sequence* family: every older symbol is the newest one with nulls.  The schedule, the gate and the policy
// are looked at before the handle, the ring after the lock is taken (ring_needed: target_batch_step_sequence_ring's rule).
static int step_sequence(const char* what, target_batch_c* b, long n_ticks, double dt, const double* dt_host, bool scheduled,
                         const void* meas_dev, long tick_stride, long ld, const unsigned char* has_meas_dev, long has_stride,
                         long ring_ticks, bool ring_needed, const target_pose_stream_c* poses, const target_innov_stream_c* innov,
                         double nis_max, const target_reacquire_c* reacq, int use_graph) {
  return guarded(what, [&] {
    const te::DtSchedule sched = scheduled ? dt_schedule(n_ticks, dt_host) : te::DtSchedule();
    const te::InnovStream stream = reacquire_stream(innov, nis_max, reacq, false);
    BatchLock lk(B(b));
    if (ring_needed && ring_ticks <= 0) throw std::invalid_argument("ring_ticks must be positive");
    if (ring_ticks < 0) throw std::invalid_argument("ring_ticks must not be negative");
    B(b)->step_sequence(n_ticks, dt, meas_dev, tick_stride, ld, has_meas_dev, has_stride, use_graph, ring_ticks, pose_stream(poses), stream, sched);
  });
}

// The target_manager_step_sequence_all* family, in the same way.  Every gate and policy is looked at before anything else is.
// streams: every symbol but the first goes through the manager's entry that refuses a negative number of batches by name.
static int step_sequence_all(const char* what, target_manager_c* m, long n_ticks, double dt, const double* dt_host, bool scheduled,
                             bool streams, const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                             const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max,
                             const target_reacquire_c* per_batch_reacq, long n_batches, int query, const double* origin, double radius,
                             int use_graph) {
  return guarded(what, [&] {
    const te::DtSchedule sched = scheduled ? dt_schedule(n_ticks, dt_host) : te::DtSchedule();
    const size_t nb = (size_t)(n_batches > 0 ? n_batches : 0);
    std::vector<te::Batch::SeqSpec> specs(nb);
    std::vector<te::PoseStream> poses(nb);
    std::vector<te::InnovStream> innov(nb);
    for (size_t i = 0; i < nb; ++i)
      innov[i] = reacquire_stream(per_batch_innov ? &per_batch_innov[i] : nullptr, per_batch_nis_max ? per_batch_nis_max[i] : 0.0,
                                  per_batch_reacq ? &per_batch_reacq[i] : nullptr, true);
    for (size_t i = 0; i < nb; ++i) {
      const target_batch_sequence_c& s = per_batch[i];
      specs[i] = te::Batch::SeqSpec{s.meas_dev, s.tick_stride, s.ld, s.has_meas_dev, s.has_stride, s.delta_dev, s.pose_dev, s.ring_ticks};
      poses[i] = pose_stream(per_batch_poses ? &per_batch_poses[i] : nullptr);
    }
    if (streams) M(m)->stepSequenceAll(n_ticks, dt, specs.data(), poses.data(), n_batches, query != 0, origin, radius, use_graph, innov.data(), sched);
    else M(m)->stepSequenceAll(n_ticks, dt, specs.data(), n_batches, query != 0, origin, radius, use_graph);
  });
}

int target_batch_step_sequence(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                               const unsigned char* has_meas_dev, long has_stride, int use_graph) {
  return step_sequence("target_batch_step_sequence", b, n_ticks, dt, nullptr, false, meas_dev, tick_stride, ld, has_meas_dev, has_stride, 0, false,
                       nullptr, nullptr, 0.0, nullptr, use_graph);
}

int target_batch_step_sequence_ring(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                                    const unsigned char* has_meas_dev, long has_stride, long ring_ticks, int use_graph) {
  return step_sequence("target_batch_step_sequence_ring", b, n_ticks, dt, nullptr, false, meas_dev, tick_stride, ld, has_meas_dev, has_stride,
                       ring_ticks, true, nullptr, nullptr, 0.0, nullptr, use_graph);
}

int target_manager_step_sequence_all(target_manager_c* m, long n_ticks, double dt, const target_batch_sequence_c* per_batch,
                                     long n_batches, int query, const double* origin, double radius, int use_graph) {
  return step_sequence_all("target_manager_step_sequence_all", m, n_ticks, dt, nullptr, false, false, per_batch, nullptr, nullptr, nullptr, nullptr,
                           n_batches, query, origin, radius, use_graph);
}

int target_manager_population_tick(target_manager_c* m) {
  int on = 0;
  const int rc = guarded("target_manager_population_tick", [&] { on = M(m)->populationTickNow() ? 1 : 0; });
  return rc < 0 ? -1 : on;
}

int target_batch_step_fused(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                            const unsigned char* has_meas_dev, long has_stride) {
  return guarded("target_batch_step_fused", [&] { BatchLock lk(B(b));
    B(b)->step_fused(n_ticks, dt, meas_dev, tick_stride, ld, has_meas_dev, has_stride);
  });
}

// ---- per-tick pose streams of launched ticks
int target_batch_step_sequence_poses(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                     long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                     const target_pose_stream_c* poses, int use_graph) {
  return step_sequence("target_batch_step_sequence_poses", b, n_ticks, dt, nullptr, false, meas_dev, tick_stride, ld, has_meas_dev, has_stride,
                       ring_ticks, false, poses, nullptr, 0.0, nullptr, use_graph);
}

int target_batch_step_fused_poses(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                                  const unsigned char* has_meas_dev, long has_stride, const target_pose_stream_c* poses) {
  return guarded("target_batch_step_fused_poses", [&] { BatchLock lk(B(b));
    B(b)->step_fused(n_ticks, dt, meas_dev, tick_stride, ld, has_meas_dev, has_stride, pose_stream(poses));
  });
}

int target_manager_step_sequence_all_poses(target_manager_c* m, long n_ticks, double dt,
                                           const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                           long n_batches, int query, const double* origin, double radius, int use_graph) {
  return step_sequence_all("target_manager_step_sequence_all_poses", m, n_ticks, dt, nullptr, false, true, per_batch, per_batch_poses, nullptr, nullptr,
                           nullptr, n_batches, query, origin, radius, use_graph);
}

// ---- per-tick innovation streams of launched ticks
int target_batch_step_sequence_innov(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                     long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                     const target_pose_stream_c* poses, const target_innov_stream_c* innov, int use_graph) {
  return step_sequence("target_batch_step_sequence_innov", b, n_ticks, dt, nullptr, false, meas_dev, tick_stride, ld, has_meas_dev, has_stride,
                       ring_ticks, false, poses, innov, 0.0, nullptr, use_graph);
}

int target_manager_step_sequence_all_innov(target_manager_c* m, long n_ticks, double dt,
                                           const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                           const target_innov_stream_c* per_batch_innov, long n_batches,
                                           int query, const double* origin, double radius, int use_graph) {
  return step_sequence_all("target_manager_step_sequence_all_innov", m, n_ticks, dt, nullptr, false, true, per_batch, per_batch_poses, per_batch_innov,
                           nullptr, nullptr, n_batches, query, origin, radius, use_graph);
}

// ---- the NIS validation gate inside launched ticks
int target_batch_step_sequence_gated(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                     long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                     const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max, int use_graph) {
  return step_sequence("target_batch_step_sequence_gated", b, n_ticks, dt, nullptr, false, meas_dev, tick_stride, ld, has_meas_dev, has_stride,
                       ring_ticks, false, poses, innov, nis_max, nullptr, use_graph);
}

int target_manager_step_sequence_all_gated(target_manager_c* m, long n_ticks, double dt,
                                           const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                           const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max, long n_batches,
                                           int query, const double* origin, double radius, int use_graph) {
  return step_sequence_all("target_manager_step_sequence_all_gated", m, n_ticks, dt, nullptr, false, true, per_batch, per_batch_poses, per_batch_innov,
                           per_batch_nis_max, nullptr, n_batches, query, origin, radius, use_graph);
}

// ---- re-acquisition of lost tracks inside the gated ticks
int target_batch_step_sequence_reacquire(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride,
                                         long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                         const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                                         const target_reacquire_c* reacq, int use_graph) {
  return step_sequence("target_batch_step_sequence_reacquire", b, n_ticks, dt, nullptr, false, meas_dev, tick_stride, ld, has_meas_dev, has_stride,
                       ring_ticks, false, poses, innov, nis_max, reacq, use_graph);
}

// ---- the gate, the innovation stream and the re-acquisition inside a launched fused call
int target_batch_step_fused_gated(target_batch_c* b, long n_ticks, double dt, const void* meas_dev, long tick_stride, long ld,
                                  const unsigned char* has_meas_dev, long has_stride,
                                  const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                                  const target_reacquire_c* reacq) {
  return guarded("target_batch_step_fused_gated", [&] {
    const te::InnovStream stream = reacquire_stream(innov, nis_max, reacq, false);
    BatchLock lk(B(b));
    B(b)->step_fused_gated(n_ticks, dt, meas_dev, tick_stride, ld, has_meas_dev, has_stride, pose_stream(poses), stream);
  });
}

int target_batch_step_fused_gate_served(target_batch_c* b) {
  return guarded_value<int>("target_batch_step_fused_gate_served", -1, [&] { BatchLock lk(B(b)); return B(b)->fused_gate_served() ? 1 : 0; });
}

int target_manager_step_sequence_all_reacquire(target_manager_c* m, long n_ticks, double dt,
                                               const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                               const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max,
                                               const target_reacquire_c* per_batch_reacq, long n_batches,
                                               int query, const double* origin, double radius, int use_graph) {
  return step_sequence_all("target_manager_step_sequence_all_reacquire", m, n_ticks, dt, nullptr, false, true, per_batch, per_batch_poses,
                           per_batch_innov, per_batch_nis_max, per_batch_reacq, n_batches, query, origin, radius, use_graph);
}

// ---- step sequences and fused replays with a time step per tick
int target_batch_step_sequence_dt(target_batch_c* b, long n_ticks, const double* dt_host, const void* meas_dev, long tick_stride,
                                  long ld, const unsigned char* has_meas_dev, long has_stride, long ring_ticks,
                                  const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                                  const target_reacquire_c* reacq, int use_graph) {
  return step_sequence("target_batch_step_sequence_dt", b, n_ticks, 0.0, dt_host, true, meas_dev, tick_stride, ld, has_meas_dev, has_stride,
                       ring_ticks, false, poses, innov, nis_max, reacq, use_graph);
}

int target_batch_step_fused_dt(target_batch_c* b, long n_ticks, const double* dt_host, const void* meas_dev, long tick_stride, long ld,
                               const unsigned char* has_meas_dev, long has_stride,
                               const target_pose_stream_c* poses, const target_innov_stream_c* innov, double nis_max,
                               const target_reacquire_c* reacq) {
  return guarded("target_batch_step_fused_dt", [&] {
    const te::DtSchedule sched = dt_schedule(n_ticks, dt_host);
    const te::InnovStream stream = reacquire_stream(innov, nis_max, reacq, false);
    BatchLock lk(B(b));
    B(b)->step_fused_gated(n_ticks, 0.0, meas_dev, tick_stride, ld, has_meas_dev, has_stride, pose_stream(poses), stream, sched);
  });
}

int target_batch_step_fused_dt_served(target_batch_c* b, int gated) {
  return guarded_value<int>("target_batch_step_fused_dt_served", -1, [&] { BatchLock lk(B(b)); return B(b)->fused_dt_served(gated != 0) ? 1 : 0; });
}

long target_batch_graph_recordings(target_batch_c* b) {
  return guarded_value<long>("target_batch_graph_recordings", -1, [&]() -> long { BatchLock lk(B(b)); return B(b)->graph_recordings(); });
}

int target_manager_step_sequence_all_dt(target_manager_c* m, long n_ticks, const double* dt_host,
                                        const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                                        const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max,
                                        const target_reacquire_c* per_batch_reacq, long n_batches,
                                        int query, const double* origin, double radius, int use_graph) {
  return step_sequence_all("target_manager_step_sequence_all_dt", m, n_ticks, 0.0, dt_host, true, true, per_batch, per_batch_poses, per_batch_innov,
                           per_batch_nis_max, per_batch_reacq, n_batches, query, origin, radius, use_graph);
}

// ---- one launch for a temporally fused replay of a whole manager
static int step_fused_all(const char* what, target_manager_c* m, long n_ticks, double dt, const double* dt_host, bool scheduled,
                          const target_batch_sequence_c* per_batch, const target_pose_stream_c* per_batch_poses,
                          const target_innov_stream_c* per_batch_innov, const double* per_batch_nis_max,
                          const target_reacquire_c* per_batch_reacq, long n_batches) {
  return guarded(what, [&] {
    TargetManager* mgr = M(m);
    const te::DtSchedule sched = scheduled ? dt_schedule(n_ticks, dt_host) : te::DtSchedule();
    const size_t nb = (size_t)(n_batches > 0 ? n_batches : 0);
    if (nb > 0 && !per_batch) throw std::invalid_argument("per_batch must not be NULL");
    std::vector<te::Batch::SeqSpec> specs(nb);
    for (size_t i = 0; i < nb; ++i) {   // (every gate and policy is looked at before anything else is)
      const target_batch_sequence_c& s = per_batch[i];
      if (s.ring_ticks != 0) throw std::invalid_argument("a fused call reads its measurements linearly: ring_ticks must be 0");
      specs[i] = te::Batch::SeqSpec{s.meas_dev, s.tick_stride, s.ld, s.has_meas_dev, s.has_stride, nullptr, nullptr, 0};
      specs[i].poses = pose_stream(per_batch_poses ? &per_batch_poses[i] : nullptr);
      specs[i].innov = reacquire_stream(per_batch_innov ? &per_batch_innov[i] : nullptr, per_batch_nis_max ? per_batch_nis_max[i] : 0.0,
                                        per_batch_reacq ? &per_batch_reacq[i] : nullptr, true);
    }
    mgr->stepFusedAll(n_ticks, dt, specs.data(), n_batches, sched);
  });
}

int target_manager_step_fused_all(target_manager_c* m, long n_ticks, double dt, const target_batch_sequence_c* per_batch,
                                  const target_pose_stream_c* per_batch_poses, const target_innov_stream_c* per_batch_innov,
                                  const double* per_batch_nis_max, const target_reacquire_c* per_batch_reacq, long n_batches) {
  return step_fused_all("target_manager_step_fused_all", m, n_ticks, dt, nullptr, false, per_batch, per_batch_poses, per_batch_innov, per_batch_nis_max,
                        per_batch_reacq, n_batches);
}

int target_manager_step_fused_all_dt(target_manager_c* m, long n_ticks, const double* dt_host, const target_batch_sequence_c* per_batch,
                                     const target_pose_stream_c* per_batch_poses, const target_innov_stream_c* per_batch_innov,
                                     const double* per_batch_nis_max, const target_reacquire_c* per_batch_reacq, long n_batches) {
  return step_fused_all("target_manager_step_fused_all_dt", m, n_ticks, 0.0, dt_host, true, per_batch, per_batch_poses, per_batch_innov, per_batch_nis_max,
                        per_batch_reacq, n_batches);
}

int target_manager_step_fused_all_served(target_manager_c* m, int gated, int scheduled) {
  return guarded_value<int>("target_manager_step_fused_all_served", -1, [&] { return M(m)->fusedAllServed(gated != 0, scheduled != 0); });
}

int target_batch_rejection_runs(target_batch_c* b, unsigned char* runs_host) {
  return guarded("target_batch_rejection_runs", [&] {
    BatchLock lk(B(b));
    if (!runs_host) throw std::invalid_argument("runs_host must not be NULL");
    B(b)->rejection_runs(runs_host);
  });
}

int target_manager_get_rejection_run(target_manager_c* m, unsigned int id) {
  int run = -1;
  const int rc = guarded("target_manager_get_rejection_run", [&] { run = M(m)->getRejectionRun(id); });
  return rc < 0 ? rc : run;
}

// ---- track lifecycle (lifecycle.hpp).  What does not depend on the handle is refused before the handle is looked at.
int target_manager_lifecycle(target_manager_c* m, const double* det_dev, const int* slot_of_det_dev, long M,
                             const unsigned char* const* has_meas_dev, long n_batches, const target_lifecycle_c* policy,
                             unsigned int* retired_ids_out, long retired_cap, long* info) {
  return guarded("target_manager_lifecycle", [&] {
    te::LifecyclePolicy p;
    if (policy) {
      p.max_misses = policy->max_misses; p.birth_type = policy->birth_type; p.first_id = policy->first_id; p.max_births = policy->max_births;
      p.dt0 = policy->dt0; p.t_birth = policy->t_birth; p.Q = policy->Q; p.R = policy->R; p.P0 = policy->P0;
    }
    te::check_lifecycle_args(policy ? &p : nullptr, info != nullptr, M, det_dev != nullptr, slot_of_det_dev != nullptr, n_batches,
                             has_meas_dev != nullptr, retired_cap, retired_ids_out != nullptr);
    assoc_manager(m)->lifecycle(det_dev, slot_of_det_dev, M, has_meas_dev, n_batches, p, retired_ids_out, retired_cap, info);
  });
}

// ---- duplicate tracks (track_merge.hpp).  What does not depend on the handle is refused before the handle is looked at.
int target_manager_find_duplicates_dev(target_manager_c* m, double dt, double gate, int rounds, double cell, int min_hits,
                                       const target_dup_out_c* per_batch, long n_batches, int* info_dev) {
  return guarded("target_manager_find_duplicates_dev", [&] {
    te::check_merge_args("find_duplicates", info_dev != nullptr, dt, gate, rounds, cell, min_hits, n_batches, per_batch != nullptr, 0, true);
    TargetManager* mgr = assoc_manager(m);
    std::vector<te::MergeSlotOut> outs((size_t)n_batches);
    for (long i = 0; i < n_batches; ++i) {
      outs[(size_t)i].dup = per_batch[i].dup_out_dev; outs[(size_t)i].partner_batch = per_batch[i].partner_batch_dev;
      outs[(size_t)i].partner_slot = per_batch[i].partner_slot_dev; outs[(size_t)i].d2 = per_batch[i].d2_of_slot_dev;
    }
    mgr->findDuplicatesDev(dt, gate, rounds, cell, min_hits, outs.data(), n_batches, info_dev);
  });
}

int target_manager_retire_duplicates(target_manager_c* m, double dt, double gate, int rounds, double cell, int min_hits,
                                     unsigned int* retired_ids_out, unsigned int* kept_ids_out, long cap, long* info) {
  return guarded("target_manager_retire_duplicates", [&] {
    te::check_merge_args("retire_duplicates", info != nullptr, dt, gate, rounds, cell, min_hits, 0, true, cap,
                         retired_ids_out != nullptr && kept_ids_out != nullptr);
    assoc_manager(m)->retireDuplicates(dt, gate, rounds, cell, min_hits, retired_ids_out, kept_ids_out, cap, info);
  });
}

int target_batch_track_counts(target_batch_c* b, unsigned char* miss_host, unsigned char* hits_host) {
  return guarded("target_batch_track_counts", [&] {
    BatchLock lk(B(b));
    B(b)->track_counts(miss_host, hits_host);
  });
}

int target_manager_get_track_counts(target_manager_c* m, unsigned int id, int* miss, int* hits) {
  bool found = false;
  const int rc = guarded("target_manager_get_track_counts", [&] {
    if (!miss || !hits) throw std::invalid_argument("miss and hits must not be NULL");
    found = M(m)->getTrackCounts(id, *miss, *hits);
  });
  return rc < 0 ? rc : (found ? 0 : 1);
}

// ---- the update policy of the by-id paths
int target_manager_set_update_gate(target_manager_c* m, int type, double nis_max, int max_rejects) {
  return guarded("target_manager_set_update_gate", [&] {
    te::check_update_gate(nis_max, max_rejects);   // (a bad policy is refused before the handle is looked at)
    M(m)->setUpdateGate(type, nis_max, max_rejects);
  });
}
int target_manager_get_update_gate(target_manager_c* m, int type, double* nis_max, int* max_rejects) {
  return guarded("target_manager_get_update_gate", [&] {
    double g = 0.0;
    int k = -1;
    if (!M(m)->getUpdateGate(type, g, k)) throw std::invalid_argument("update gate: no such model type");
    if (nis_max) *nis_max = g;
    if (max_rejects) *max_rejects = k;
  });
}
int target_manager_update_gate_served(target_manager_c* m, int type) {
  return guarded_value<int>("target_manager_update_gate_served", -1, [&] { return M(m)->updateGateServed(type); });
}
long target_manager_update_meas_batch_gated(target_manager_c* m, const unsigned int* ids, long n, double dt, const double* meas,
                                            const unsigned char* has_meas, double* nis_out, unsigned char* event_out) {
  long k = -1;
  guarded("target_manager_update_meas_batch_gated", [&] { k = M(m)->updateBatch(ids, n, dt, meas, has_meas, nis_out, event_out); });
  return k;
}

// ---- resident ("live") mode
int target_batch_live_start(target_batch_c* b, double dt, const void* meas_ring_dev, long tick_stride, long ld,
                            const unsigned char* has_ring_dev, long has_stride, long ring_ticks, long first_entry, long max_ticks,
                            double idle_limit_s) {
  return guarded("target_batch_live_start", [&] { BatchLock lk(B(b));
    B(b)->live_start(dt, meas_ring_dev, tick_stride, ld, has_ring_dev, has_stride, ring_ticks, first_entry, max_ticks, idle_limit_s);
  });
}
int target_batch_live_set_pose_output(target_batch_c* b, double* pose_soa_dev, long ld) {
  return guarded("target_batch_live_set_pose_output", [&] { BatchLock lk(B(b)); B(b)->live_set_pose_output(pose_soa_dev, ld); });
}
int target_batch_live_set_gate(target_batch_c* b, double nis_max, const target_innov_stream_c* nis, const target_reacquire_c* reacq) {
  return guarded("target_batch_live_set_gate", [&] {
    if (!(nis_max >= 0.0)) throw std::invalid_argument("live gate: nis_max must be 0 (no gate) or positive, got " + std::to_string(nis_max));
    te::InnovStream g;
    if (nis_max > 0.0 && nis) {
      if (!nis->nis_dev) throw std::invalid_argument("live gate: nis_max > 0 needs the NIS rows of the session (nis_dev): they report the decisions");
      if (nis->innov_dev) throw std::invalid_argument("live gate: the innovations are not served in resident sessions (innov_dev must be NULL)");
      g = reacquire_stream(nis, nis_max, reacq, false);
      if (reacq && reacq->event_dev == nullptr) { g.reacq.ld = 0; g.reacq.tick_stride = 0; g.reacq.ring = 0; }
    } else if (reacq) {
      throw std::invalid_argument("live gate: a policy needs the gate (nis_max > 0 and the NIS rows): it counts the gate's rejections");
    }
    BatchLock lk(B(b));
    B(b)->live_set_gate(g);
  });
}
int target_batch_live_gate_served(target_batch_c* b) {
  return guarded_value<int>("target_batch_live_gate_served", -1, [&] { BatchLock lk(B(b)); return B(b)->live_gate_refusal() == nullptr ? 1 : 0; });
}
int target_batch_live_post(target_batch_c* b, long n_ticks) {
  return guarded("target_batch_live_post", [&] { BatchLock lk(B(b)); B(b)->live_post(n_ticks); });
}
int target_batch_live_post_each(target_batch_c* b, long n_ticks) {
  return guarded("target_batch_live_post_each", [&] { BatchLock lk(B(b)); for (long i = 0; i < n_ticks; ++i) B(b)->live_post(1); });
}
long target_batch_live_done(target_batch_c* b) {
  return guarded_value<long>("target_batch_live_done", -1L, [&] { return B(b)->live_done(); });   // reads host-mapped words: no lock
}
int target_batch_live_wait(target_batch_c* b, long tick, double timeout_s) {
  int late = 0;
  const int rc = guarded("target_batch_live_wait", [&] { late = B(b)->live_wait(tick, timeout_s) ? 0 : 1; });
  return rc != 0 ? rc : late;
}
long target_batch_live_stop(target_batch_c* b) {
  return guarded_value<long>("target_batch_live_stop", -1L, [&] { BatchLock lk(B(b)); return B(b)->live_stop(); });
}
int target_batch_live_running(target_batch_c* b) {
  return guarded_value<int>("target_batch_live_running", -1, [&] { return B(b)->live_running() ? 1 : 0; });   // reads a host-mapped word: no lock
}
long target_batch_live_capacity(target_batch_c* b) {
  return guarded_value<long>("target_batch_live_capacity", -1L, [&] { return B(b)->live_capacity_next(); });
}

int target_manager_live_start_all(target_manager_c* m, double dt, const target_batch_sequence_c* per_batch, long n_batches, long first_entry,
                                  long max_ticks, double idle_limit_s, int query, const double* origin, double radius) {
  return guarded("target_manager_live_start_all", [&] {
    if (!per_batch || n_batches <= 0) throw std::invalid_argument("NULL per-batch description");
    std::vector<Batch::SeqSpec> specs((size_t)n_batches);
    for (long i = 0; i < n_batches; ++i)
      specs[(size_t)i] = Batch::SeqSpec{per_batch[i].meas_dev, per_batch[i].tick_stride, per_batch[i].ld, per_batch[i].has_meas_dev,
                                        per_batch[i].has_stride, per_batch[i].delta_dev, per_batch[i].pose_dev, per_batch[i].ring_ticks};
    M(m)->liveStartAll(dt, specs.data(), n_batches, first_entry, max_ticks, idle_limit_s, query != 0, origin, radius);
  });
}
int target_manager_live_post_all(target_manager_c* m, long n_ticks, int one_doorbell_per_tick) {
  return guarded("target_manager_live_post_all", [&] { M(m)->livePostAll(n_ticks, one_doorbell_per_tick != 0); });
}
long target_manager_live_done_all(target_manager_c* m) {
  return guarded_value<long>("target_manager_live_done_all", -1L, [&] { return M(m)->liveDoneAll(); });
}
int target_manager_live_wait_all(target_manager_c* m, long tick, double timeout_s) {
  int late = 0;
  const int rc = guarded("target_manager_live_wait_all", [&] { late = M(m)->liveWaitAll(tick, timeout_s) ? 0 : 1; });
  return rc != 0 ? rc : late;
}
long target_manager_live_stop_all(target_manager_c* m) {
  return guarded_value<long>("target_manager_live_stop_all", -1L, [&] { return M(m)->liveStopAll(); });
}

int target_batch_get_est_dev(target_batch_c* b, double* pose_dev, double* twist_dev, double* acc_dev, int at_time, double t1) {
  return guarded("target_batch_get_est_dev", [&] { BatchLock lk(B(b)); B(b)->outputs_dev(pose_dev, twist_dev, acc_dev, at_time != 0, t1); });
}

int target_batch_pack_meas_dev(target_batch_c* b, const double* meas_aos_dev, long n, void* meas_soa_dev, long ld) {
  return guarded("target_batch_pack_meas_dev", [&] { BatchLock lk(B(b)); B(b)->pack_meas_dev(meas_aos_dev, n, meas_soa_dev, ld); });
}

// ---------------------------------------------------------------- pose gather over xGMI (RCCL)
int target_comm_unique_id(char* out128) {
  return guarded("target_comm_unique_id", [&] {
    if (!out128) throw std::invalid_argument("NULL buffer");
    te::PoseComm::unique_id(out128);
  });
}

target_comm_c* target_comm_new(const char* id128, int rank, int world) {
  te::PoseComm* c = nullptr;
  guarded("target_comm_new", [&] {
    if (!id128) throw std::invalid_argument("NULL id");
    c = new te::PoseComm(id128, rank, world);
  });
  return (target_comm_c*)c;
}

void target_comm_delete(target_comm_c* comm) {
  if (comm) guarded("target_comm_delete", [&] { delete (te::PoseComm*)comm; });
}

int target_manager_gather_pose_begin(target_manager_c* self, target_comm_c* comm, int root, const long* counts, double* recv_dev) {
  return guarded("target_manager_gather_pose_begin", [&] {
    if (M(self)->numShards() > 1) throw std::runtime_error("the RCCL gather is refused on a manager with more than one shard");
    if (!comm || !counts) throw std::invalid_argument("NULL communicator or counts");
    ((te::PoseComm*)comm)->begin(M(self), root, counts, recv_dev);
  });
}

int target_manager_gather_pose_wait(target_comm_c* comm, float* device_ms) {
  return guarded("target_manager_gather_pose_wait", [&] {
    if (!comm) throw std::invalid_argument("NULL communicator");
    ((te::PoseComm*)comm)->wait();
    if (device_ms) *device_ms = ((te::PoseComm*)comm)->last_ms();
  });
}

int target_manager_gather_pose_wait_for(target_comm_c* comm, double timeout_s, float* device_ms) {
  int pending = 0;
  const int rc = guarded("target_manager_gather_pose_wait_for", [&] {
    if (!comm) throw std::invalid_argument("NULL communicator");
    if (!((te::PoseComm*)comm)->wait_for(timeout_s)) { pending = 1; return; }
    if (device_ms) *device_ms = ((te::PoseComm*)comm)->last_ms();
  });
  return rc != 0 ? rc : pending;
}

// ---------------------------------------------------------------- measurement ingest
target_ingest_c* target_ingest_new(target_manager_c* manager, int type, const double* Q, const double* R, const double* P0) {
  te::MeasurementIngest* ing = nullptr;
  guarded("target_ingest_new", [&] { ing = new te::MeasurementIngest(M(manager), type, Q, R, P0); });
  return (target_ingest_c*)ing;
}

void target_ingest_delete(target_ingest_c* ingest) {
  if (ingest) guarded("target_ingest_delete", [&] { delete (te::MeasurementIngest*)ingest; });
}

void target_ingest_set_expiration_time(target_ingest_c* ingest, double seconds) {
  guarded("target_ingest_set_expiration_time", [&] { I(ingest)->setExpirationTime(seconds); });
}

void target_ingest_set_token_name(target_ingest_c* ingest, const char* token) {
  guarded("target_ingest_set_token_name", [&] { I(ingest)->setTargetTokenName(token); });
}

int target_ingest_push(target_ingest_c* ingest, unsigned int id, double stamp, const double* pose) {
  return guarded("target_ingest_push", [&] { I(ingest)->push(id, stamp, pose); });
}

int target_ingest_push_named(target_ingest_c* ingest, const char* child_frame_id, double stamp, const double* pose) {
  int r = -2;
  guarded("target_ingest_push_named", [&] { r = I(ingest)->push_named(child_frame_id, stamp, pose); });
  return r;
}

long target_ingest_tick(target_ingest_c* ingest, double dt, double now, unsigned int* ids_out, double* poses_out, long capacity) {
  long n = -1;
  guarded("target_ingest_tick", [&] {
    std::vector<unsigned> ids;
    std::vector<double> poses;
    n = I(ingest)->tick(dt, now, ids, poses);
    for (long i = 0; i < n && i < capacity; ++i) {
      if (ids_out) ids_out[i] = ids[(size_t)i];
      if (poses_out) for (int c = 0; c < 7; ++c) poses_out[i * 7 + c] = poses[(size_t)i * 7 + c];
    }
  });
  return n;
}

// ---------------------------------------------------------------- IntersectionSolver as an object
target_intersection_solver_c* target_intersection_solver_new(target_manager_c* manager, unsigned int filters_length) {
  te::IntersectionSolver* sv = nullptr;
  guarded("target_intersection_solver_new", [&] { sv = new te::IntersectionSolver(M(manager), filters_length); });
  return (target_intersection_solver_c*)sv;
}
void target_intersection_solver_delete(target_intersection_solver_c* solver) {
  if (solver) guarded("target_intersection_solver_delete", [&] { delete (te::IntersectionSolver*)solver; });
}
double target_intersection_solver_get_time_with_sphere(target_intersection_solver_c* solver, unsigned int id, double t1,
                                                        const double* origin, double radius) {
  return guarded_value<double>("target_intersection_solver_get_time_with_sphere", -1.0, [&] {
    if (!solver || !origin) throw std::invalid_argument("NULL argument");
    return ((te::IntersectionSolver*)solver)->getIntersectionTimeWithSphere(id, t1, origin, radius);
  });
}
bool target_intersection_solver_get_pose_with_sphere(target_intersection_solver_c* solver, unsigned int id, double t1, double pos_th,
                                                     double ang_th, const double* origin, double radius, double* pose7) {
  return guarded_value<bool>("target_intersection_solver_get_pose_with_sphere", false, [&] {
    if (!solver || !origin || !pose7) throw std::invalid_argument("NULL argument");
    return ((te::IntersectionSolver*)solver)->getIntersectionPoseWithSphere(id, t1, pos_th, ang_th, origin, radius, pose7);
  });
}
void target_intersection_solver_last_errors(target_intersection_solver_c* solver, double* pos_error_filtered, double* ang_error_filtered) {
  if (!solver) return;
  if (pos_error_filtered) *pos_error_filtered = ((te::IntersectionSolver*)solver)->lastPositionErrorFiltered();
  if (ang_error_filtered) *ang_error_filtered = ((te::IntersectionSolver*)solver)->lastAngleErrorFiltered();
}

// ---------------------------------------------------------------- TargetInterface / estimator getters
int target_manager_set_shared_axes(target_manager_c* self, int on) {
  return guarded("target_manager_set_shared_axes", [&] { M(self)->setSharedAxes(on != 0); });
}
int target_manager_set_uniform_tiles(target_manager_c* self, int on) {
  return guarded("target_manager_set_uniform_tiles", [&] { M(self)->setUniformTiles(on != 0); });
}
int target_manager_set_keep_measurement(target_manager_c* self, int on) {
  return guarded("target_manager_set_keep_measurement", [&] { M(self)->setKeepMeasurement(on != 0); });
}
bool target_manager_get_measured_pose(target_manager_c* self, unsigned int id, double* pose7) {
  return guarded_value<bool>("target_manager_get_measured_pose", false, [&] { return M(self)->getTargetMeasuredPose(id, pose7); });
}
bool target_manager_get_period_estimate(target_manager_c* self, unsigned int id, double* period) {
  return guarded_value<bool>("target_manager_get_period_estimate", false, [&] {
    double p = -1.0;
    const bool ok = M(self)->getTargetPeriodEstimate(id, p);
    if (ok && period) *period = p;
    return ok;
  });
}
bool target_manager_get_estimated_transform(target_manager_c* self, unsigned int id, double* T16) {
  return guarded_value<bool>("target_manager_get_estimated_transform", false, [&] { return M(self)->getTargetTransform(id, T16); });
}
int target_manager_get_n(target_manager_c* self, unsigned int id) {
  return guarded_value<int>("target_manager_get_n", -1, [&] { int n = 0, m = 0; return M(self)->getTargetDims(id, n, m) ? n : 0; });
}
int target_manager_get_m(target_manager_c* self, unsigned int id) {
  return guarded_value<int>("target_manager_get_m", -1, [&] { int n = 0, m = 0; return M(self)->getTargetDims(id, n, m) ? m : 0; });
}
bool target_manager_get_model_matrices(target_manager_c* self, unsigned int id, double* Q, double* R, double* P0) {
  return guarded_value<bool>("target_manager_get_model_matrices", false, [&] { return M(self)->getTargetModelMatrices(id, Q, R, P0); });
}
int target_manager_set_log_targets(target_manager_c* self, const unsigned int* ids, long n) {
  return guarded("target_manager_set_log_targets", [&] {
    if (n > 0 && !ids) throw std::invalid_argument("NULL id list");
    M(self)->setLogTargets(ids, n);
  });
}

// ---------------------------------------------------------------- one manager over several devices
int target_manager_set_devices(target_manager_c* m, const int* devices, int n) {
  return guarded("target_manager_set_devices", [&] { M(m)->setDevices(devices, n); });
}
int target_manager_num_shards(target_manager_c* m) {
  return guarded_value<int>("target_manager_num_shards", -1, [&] { return M(m)->numShards(); });
}
int target_manager_shard_device(target_manager_c* m, int k) {
  return guarded_value<int>("target_manager_shard_device", -1, [&] { return M(m)->shardDevice(k); });
}
int target_manager_shard_of(target_manager_c* m, unsigned int id) {
  return guarded_value<int>("target_manager_shard_of", -1, [&] { return M(m)->shardOf(id); });
}
int target_manager_batch_shard(target_manager_c* m, int index) {
  return guarded_value<int>("target_manager_batch_shard", -1, [&] { return M(m)->batchShard(index); });
}
int target_manager_set_shard_stream(target_manager_c* m, int k, void* hip_stream) {
  return guarded("target_manager_set_shard_stream", [&] { M(m)->setShardStream(k, (hipStream_t)hip_stream); });
}
long target_manager_get_est_all_by_id(target_manager_c* m, double* pose_out, long capacity) {
  return guarded_value<long>("target_manager_get_est_all_by_id", -1L, [&] { return M(m)->getEstAllById(pose_out, capacity); });
}

// ---------------------------------------------------------------- synthetic measurement streams
int target_stream_fill_dev(const target_stream_c* sp, long n_targets, long first_tick, long n_ticks, int dtype, void* meas_dev,
                           long tick_stride, long ld, unsigned char* has_meas_dev, long has_stride, void* hip_stream) {
  return guarded("target_stream_fill_dev", [&] {
    if (!sp) throw std::invalid_argument("NULL stream description");
    if (dtype != TARGET_DTYPE_F64 && dtype != TARGET_DTYPE_F32) throw std::invalid_argument("unknown dtype");
    te::stream_fill(te::StreamSpec{sp->model, (uint64_t)sp->seed, sp->first_target, sp->dt, sp->availability, sp->rpy_noise}, n_targets,
                    first_tick, n_ticks, dtype == TARGET_DTYPE_F32, meas_dev, tick_stride, ld, has_meas_dev, has_stride, (hipStream_t)hip_stream);
  });
}

int target_stream_truth_dev(const target_stream_c* sp, long n_targets, double* pose0_dev, double* truth_dev, void* hip_stream) {
  return guarded("target_stream_truth_dev", [&] {
    if (!sp) throw std::invalid_argument("NULL stream description");
    te::stream_truth(te::StreamSpec{sp->model, (uint64_t)sp->seed, sp->first_target, sp->dt, sp->availability, sp->rpy_noise}, n_targets,
                     pose0_dev, truth_dev, (hipStream_t)hip_stream);
  });
}

}  // extern "C"
