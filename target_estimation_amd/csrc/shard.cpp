// shard.cpp -- see shard.hpp.
#include "shard.hpp"
#include "id_resolve.hpp"
#include "kf_population.hpp"
#include "shard_map.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>

#include "hip_check.hpp"

namespace te {

static const double kZero6[6] = {0, 0, 0, 0, 0, 0};

Shard::Shard(const ShardSettings& settings, std::mutex* owner_lock) : set_(settings), owner_lock_(owner_lock) {}

Shard::~Shard() { dropSeqGraphs(); }   // (everything else is the members': shard.hpp on their order)

void Shard::devIdsReserve(long n) {
  DevIds& d = dev_ids_;
  if (!d.h_counters) {   // (the pinned word last: its presence stands for both)
    d.counters.alloc(1);
    d.h_counters.alloc(1);
  }
  if (n <= d.cap) return;
  const long want = std::max(n, d.cap * 2);
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  // (nothing to carry over: released before the new blocks exist; a throw leaves an empty staging area)
  d.cap = 0;
  d.ids.reset(); d.loc.reset(); d.idx.reset(); d.aos.reset(); d.soa.reset();
  d.mask.reset(); d.found.reset(); d.out.reset(); d.gnis.reset(); d.gev.reset();
  d.gnis.alloc((size_t)want);
  d.gev.alloc((size_t)want);
  d.ids.alloc((size_t)want);
  d.loc.alloc((size_t)want);
  d.idx.alloc((size_t)want);
  d.aos.alloc(7 * (size_t)want);
  d.soa.alloc((set_.dtype == F64 ? 8 : 4) * 7 * (size_t)want);
  d.mask.alloc((size_t)want);
  d.found.alloc((size_t)want);
  d.out.alloc(19 * (size_t)want);
  d.cap = want;
}

void Shard::devIdsRebuild() {
  DevIds& d = dev_ids_;
  const size_t total = targets_.size();
  int log2cap = 4;
  while ((size_t(1) << log2cap) < 2 * total + 16) ++log2cap;
  if (log2cap > 31) throw std::runtime_error("target_estimation_amd: too many targets for the device id table");
  if (log2cap != d.log2cap) {
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    const size_t cap = size_t(1) << log2cap;
    DeviceBuf<unsigned> keys, vals;
    DeviceBuf<int> seen;
    keys.alloc(cap);
    vals.alloc(cap);
    seen.alloc(cap);
    d.keys = std::move(keys); d.vals = std::move(vals); d.seen = std::move(seen);
    d.log2cap = log2cap;
  }
  const size_t cap = size_t(1) << d.log2cap;
  TE_HIP_CHECK(hipMemsetAsync(d.vals.get(), 0xFF, sizeof(unsigned) * cap, stream_));
  TE_HIP_CHECK(hipMemsetAsync(d.seen.get(), 0, sizeof(int) * cap, stream_));
  d.epoch = 0;
  for (size_t b = 0; b < batches_.size(); ++b) {
    const long n = batches_[b]->size();
    if (!n) continue;
    devIdsReserve(n);
    TE_HIP_CHECK(hipMemcpyAsync(d.ids.get(), batches_[b]->slot_ids().data(), sizeof(unsigned) * n, hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL(id_table_insert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d.keys.get(), d.vals.get(), d.log2cap,
                       d.ids.get(), n, (unsigned)b);
    TE_HIP_CHECK(hipGetLastError());
    TE_HIP_CHECK(hipStreamSynchronize(stream_));   // d.ids is reused by the next batch; slot_ids() is pageable memory
  }
  d.dirty = false;
}

bool Shard::resolveOnDevice(const unsigned* ids, long n, ResolveCounters& out) {
  if (batches_.empty() || batches_.size() > (size_t)kIdMaxBatches) return false;
  for (auto& b : batches_)
    if (b->size() >= (1L << kIdSlotBits)) return false;
  DevIds& d = dev_ids_;
  if (d.dirty) devIdsRebuild();
  devIdsReserve(n);
  if (++d.epoch == 0x7fffffff) { TE_HIP_CHECK(hipMemsetAsync(d.seen.get(), 0, sizeof(int) * (size_t(1) << d.log2cap), stream_)); d.epoch = 1; }
  TE_HIP_CHECK(hipMemcpyAsync(d.ids.get(), ids, sizeof(unsigned) * n, hipMemcpyHostToDevice, stream_));
  TE_HIP_CHECK(hipMemsetAsync(d.counters.get(), 0, sizeof(ResolveCounters), stream_));
  hipLaunchKernelGGL(id_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d.keys.get(), d.vals.get(), d.seen.get(), d.log2cap,
                     d.ids.get(), n, d.epoch, d.loc.get(), d.counters.get());
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipMemcpyAsync(d.h_counters.host(), d.counters.get(), sizeof(ResolveCounters), hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  out = *d.h_counters.host();
  return true;
}

bool is_axis_separable(int type, const double* Q, const double* R, const double* P0, long n_P0) {
  const int n = model_n(type), m = model_m(type);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      if (group_of(type, r) == group_of(type, c)) continue;
      if (Q[r * n + c] != 0.0) return false;
      for (long k = 0; k < n_P0; ++k)
        if (P0[k * n * n + r * n + c] != 0.0) return false;
    }
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c)
      if (group_of(type, r) != group_of(type, c) && R[r * m + c] != 0.0) return false;
  return true;
}

bool axes_shareable(int type, const double* Q, const double* R, const double* P0, long n_P0) {
  return is_axis_separable(type, Q, R, P0, n_P0) && shared_axes_qr_ok(type, Q, R) && shared_axes_p0_ok(type, P0, n_P0);
}

// exact symmetry of Q, R and every P0 (covariances are; the reference accepts any matrix)
static bool all_symmetric(int type, const double* Q, const double* R, const double* P0, long n_P0) {
  const int n = model_n(type), m = model_m(type);
  for (int r = 0; r < n; ++r)
    for (int c = r + 1; c < n; ++c) {
      if (Q[r * n + c] != Q[c * n + r]) return false;
      for (long k = 0; k < n_P0; ++k)
        if (P0[k * n * n + r * n + c] != P0[k * n * n + c * n + r]) return false;
    }
  for (int r = 0; r < m; ++r)
    for (int c = r + 1; c < m; ++c)
      if (R[r * m + c] != R[c * m + r]) return false;
  return true;
}

int Shard::chooseLayout(int type, const double* Q, const double* R, const double* P0, long n_P0) const {
  constexpr int kSeparable = 201;        // 1 + TARGET_LAYOUT_AXIS_SEPARABLE
  constexpr int kSeparablePacked = 301;  // 1 + TARGET_LAYOUT_AXIS_SEPARABLE_PACKED
  const bool sep = is_axis_separable(type, Q, R, P0, n_P0);
  // automatic: the smallest record the matrices allow -- per-axis-group blocks when nothing couples the
  // groups, their upper triangles only when everything is symmetric as well
  if (set_.lanes == 0) {
    const bool sym = all_symmetric(type, Q, R, P0, n_P0);
    if (sep) return sym ? kSeparablePacked : kSeparable;
    if (!sym) return 0;   // general matrices: dense kernel, full P, tuned lanes per target
    // coupled but symmetric: dense kernel on the upper triangle (100 + lanes per target): per (model, precision) the
    // fastest packed form at 10^6 targets (profiles/r02_layout_sweep.txt, profiles/r02_kernel_resources.txt).
    //   angular_velocities: 101 = thread per target on the triangle in place (ekf_sym.hpp): 309 us fp64 / 190 us fp32 per
    //     10^6-target tick against 493 / 212 us for the best lanes-per-target form (106 / 103);
    //   angular_rates: fp64 106 held to two wavefronts per SIMD (kf_step.hpp step_min_waves: 647 us; 103 takes 714 us at
    //     one wavefront), fp32 103 (299 us).
    // The AV picks run at one wavefront per SIMD: they are the fastest forms measured, their two-wave alternatives lose 10-60 %.
    switch (type) {
      case ANGULAR_RATES: return set_.dtype == F32 ? 103 : 106;
      case ANGULAR_VELOCITIES: return 101;
      case UNIFORM_ACCELERATION: return set_.dtype == F32 ? 103 : 101;
      default: return 101;
    }
  }
  if ((set_.lanes == kSeparable || set_.lanes == kSeparablePacked) && !sep)
    throw std::runtime_error("target_estimation_amd: the axis-separable layout was requested but Q, R or P0 couple different axes");
  return set_.lanes;
}

int Shard::findOrCreateBatch(int type, const double* Q, const double* R, int lanes_code, int& cls) {
  // a batch per (model, layout): at most a handful, so a scan; the (Q, R) class inside it is a hash lookup
  for (size_t b = 0; b < batches_.size(); ++b)
    if (batches_[b]->type() == type && batches_[b]->lanes_code() == lanes_code) {
      cls = batches_[b]->find_class(Q, R);
      if (cls < 0) cls = batches_[b]->add_class(Q, R);
      return (int)b;
    }
  // (the batch itself decides from Q and R whether it starts in the shared-axes form, and from every P0 whether it stays in it)
  batches_.emplace_back(new Batch(type, set_.dtype, lanes_code, Q, R, stream_, owner_lock_, set_.shared_axes, set_.uniform_tiles));
  batches_.back()->set_soonest_scratch(&soonest_, set_.soonest_max_wgs);
  batches_.back()->set_assoc_scratch(&assoc_, set_.assoc_col_chunks, set_.assoc_grid_buckets);
  if (set_.keep_meas) batches_.back()->set_keep_measurement(true);
  if (type >= 0 && type < 4 && set_.gate[type].on()) batches_.back()->set_update_gate(set_.gate[type]);
  cls = 0;
  return (int)batches_.size() - 1;
}

const Batch* Shard::batchOf(unsigned id) const {
  Loc loc;
  return find(id, loc) ? batches_[(size_t)loc.batch].get() : nullptr;
}

void Shard::notFound(unsigned id) const {
  std::cout << "Target(" << id << ") does not exist!" << std::endl;
}

template <class Before>
void Shard::splitBySlot(const unsigned* ids, long n, BySlot& by, Before&& before_each) const {
  by.sp.src.resize(batches_.size());
  by.slots.resize(batches_.size());
  for (long i = 0; i < n; ++i) {
    Loc loc;
    if (!find(ids[i], loc)) { by.sp.unknown.push_back(i); continue; }
    before_each((size_t)loc.batch, loc);
    by.slots[(size_t)loc.batch].push_back(loc.slot);
    by.sp.src[(size_t)loc.batch].push_back(i);
    ++by.known;
  }
}

// The fast path of the host-array calls: the caller passes exactly one batch's ids in slot order (the usual case when the same
// id array is reused every tick).  That batch, or null.
Batch* Shard::wholeBatch(const unsigned* ids, long n) const {
  for (const auto& b : batches_)
    if (b->size() == n && n > 0 && std::memcmp(ids, b->slot_ids().data(), sizeof(unsigned) * (size_t)n) == 0) return b.get();
  return nullptr;
}

// found[i] of a host-array call from the positions of its unknown ids
static void mark_found(unsigned char* found, long n, const std::vector<long>& unknown) {
  if (!found || n <= 0) return;
  std::memset(found, 1, (size_t)n);
  for (long i : unknown) found[i] = 0;
}

void host_quat_to_rot(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

namespace {
// rotToRpy, geometry.hpp:191-196
void host_rot_to_rpy(const double* R, double* rpy) {
  rpy[0] = std::atan2(R[7], R[8]);
  rpy[1] = std::atan2(-R[6], std::sqrt(R[7] * R[7] + R[8] * R[8]));
  rpy[2] = std::atan2(R[3], R[0]);
}
// one row in writeTxtFile's format (utils.hpp:96-120: `myfile << value << " "` per column, then "\n"; default ostream
// formatting = %g with 6 significant digits)
void append_row(std::string& out, const double* v, long w) {
  char buf[40];
  for (long c = 0; c < w; ++c) {
    std::snprintf(buf, sizeof buf, "%g ", v[c]);
    out += buf;
  }
  out += "\n";
}
}  // namespace

void Shard::keepMeasurementChanged() {
  for (auto& b : batches_) b->set_keep_measurement(set_.keep_meas);
  dropSeqGraphs();
}

// The rows of the selected ids that this shard holds, grouped by batch (batch order), in the order of `ids` inside a batch;
// LogRow::batch = the batch index.
void Shard::logCollect(const std::vector<unsigned>& ids, std::vector<LogRow>& rows) {
  BySlot by;   // (a selected target that does not exist -- yet, or any more -- is left out)
  splitBySlot(ids.data(), (long)ids.size(), by, [](size_t, const Loc&) {});
  const std::vector<std::vector<int>>& slots = by.slots;
  for (size_t bi = 0; bi < batches_.size(); ++bi) {
    Batch& b = *batches_[bi];
    const long n = (long)slots[bi].size();
    if (!n) continue;
    const int N = b.n_state();
    std::vector<double> pose((size_t)n * 7), twist((size_t)n * 6), acc((size_t)n * 6), x((size_t)n * N), P((size_t)n * N * N), meas((size_t)n * 7);
    b.outputs(slots[bi].data(), n, pose.data(), twist.data(), acc.data(), false, 0.0);
    b.get_state(slots[bi].data(), n, x.data(), P.data());
    if (b.keep_measurement()) b.measured_poses(slots[bi].data(), n, meas.data());
    else for (long s = 0; s < n; ++s) for (int c = 0; c < 7; ++c) meas[(size_t)s * 7 + c] = c == 6 ? 1.0 : 0.0;
    for (long s = 0; s < n; ++s) {
      LogRow r;
      r.id = ids[(size_t)by.sp.src[bi][(size_t)s]];
      r.batch = (int)bi;
      const double t = b.time(slots[bi][(size_t)s]);
      double R[9], pose6[6];
      host_quat_to_rot(&pose[(size_t)s * 7 + 3], R);
      for (int c = 0; c < 3; ++c) pose6[c] = pose[(size_t)s * 7 + c];
      host_rot_to_rpy(R, pose6 + 3);   // isometryToPose6d, geometry.hpp:602-608
      const double* row[7] = {&t, &meas[(size_t)s * 7], &pose[(size_t)s * 7], &twist[(size_t)s * 6], pose6, &acc[(size_t)s * 6],
                              &P[(size_t)s * N * N]};
      const long width[7] = {1, 7, 7, 6, 6, 6, (long)N * N};
      for (int ch = 0; ch < 7; ++ch) append_row(r.ch[ch], row[ch], width[ch]);
      rows.push_back(std::move(r));
    }
  }
}

bool Shard::measuredPose(unsigned id, double* pose7) {
  Loc loc;
  if (!find(id, loc) || !batches_[(size_t)loc.batch]->keep_measurement()) return false;
  const int slot = loc.slot;
  batches_[(size_t)loc.batch]->measured_poses(&slot, 1, pose7);
  return true;
}

bool Shard::dims(unsigned id, int& n, int& m) {
  Loc loc;
  if (!find(id, loc)) return false;
  n = batches_[(size_t)loc.batch]->n_state();
  m = batches_[(size_t)loc.batch]->n_meas();
  return true;
}

bool Shard::modelMatrices(unsigned id, double* Q, double* R, double* P0) {
  Loc loc;
  if (!find(id, loc)) return false;
  Batch& b = *batches_[(size_t)loc.batch];
  if (Q || R) b.class_matrices(loc.slot, Q, R);
  if (P0 && !b.initial_covariance(loc.slot, P0)) return false;
  return true;
}

bool Shard::init(int type, unsigned id, double t0, const double* Q, const double* R, const double* P0, const double* p0, const double* v0,
                 const double* a0) {
  if (targets_.contains(id)) {
    std::cout << "Target(" << id << ") already exists!" << std::endl;
    return false;
  }
  int cls = 0;
  const int b = findOrCreateBatch(type, Q, R, chooseLayout(type, Q, R, P0, 1), cls);
  const long slot = batches_[(size_t)b]->append(1, &id, t0, P0, false, p0, v0 ? v0 : kZero6, a0 ? a0 : kZero6, cls);
  targets_.set(id, Loc{b, (int)slot});
  dev_ids_.dirty = true;
  if (set_.verbose) {
    switch (type) {
      case ANGULAR_RATES: std::cout << "Using angular rates for the orientation" << std::endl; break;
      case ANGULAR_VELOCITIES: std::cout << "Using angular velocities for the orientation" << std::endl; break;
      case UNIFORM_ACCELERATION: std::cout << "Uniformly accelerated motion" << std::endl; break;
      case UNIFORM_VELOCITY: std::cout << "Uniform rectilinear motion" << std::endl; break;
    }
  }
  return true;
}

long Shard::initBatch(int type, const unsigned* ids, long n, double t0, const double* Q, const double* R, const double* P0,
                      bool per_target_P0, const double* p0, const double* v0, const double* a0) {
  const int N = model_n(type);
  const std::vector<long> keep = newIdsOnly(ids, n, [&](unsigned id) { return targets_.contains(id); }, [&](unsigned id) {
    if (set_.verbose) std::cout << "Target(" << id << ") already exists!" << std::endl;
  });
  if (keep.empty()) return 0;
  const long k = (long)keep.size();
  int cls = 0;
  const int b = findOrCreateBatch(type, Q, R, chooseLayout(type, Q, R, P0, per_target_P0 ? n : 1), cls);
  const std::vector<long>* pos = k == n ? nullptr : &keep;   // every id new: the caller's arrays as they are
  RowsIn<unsigned> ids2(ids, pos, 1);
  RowsIn<double> p2(p0, pos, 7), v2(v0, pos, 6), a2(a0, pos, 6), P2(P0, per_target_P0 ? pos : nullptr, (long)N * N);
  const long first = batches_[(size_t)b]->append(k, ids2.get(), t0, P2.get(), per_target_P0, p2.get(), v2.get(), a2.get(), cls);
  targets_.reserve(targets_.size() + (size_t)k);
  for (long j = 0; j < k; ++j) targets_.set(ids[keep[(size_t)j]], Loc{b, (int)(first + j)});
  dev_ids_.dirty = true;
  return k;
}

long Shard::initBatchClasses(int type, const unsigned* ids, long n, double t0, long n_classes, const double* Q, const double* R,
                             const double* P0, const unsigned* class_of, const double* p0, const double* v0, const double* a0) {
  const int N = model_n(type), M = model_m(type);
  // every class: its layout (the matrices decide) -> batch, and its index inside that batch
  std::vector<int> cls_batch((size_t)n_classes), cls_idx((size_t)n_classes);
  for (long c = 0; c < n_classes; ++c) {
    const double* Qc = Q + c * N * N;
    const double* Rc = R + c * M * M;
    const double* Pc = P0 + c * N * N;
    cls_batch[(size_t)c] = findOrCreateBatch(type, Qc, Rc, chooseLayout(type, Qc, Rc, Pc, 1), cls_idx[(size_t)c]);
  }
  for (long i = 0; i < n; ++i)
    if (class_of[i] >= (unsigned long)n_classes) throw std::invalid_argument("target_estimation_amd: class index out of range");
  // new ids only, grouped by destination batch in input order
  const std::vector<long> keep = newIdsOnly(ids, n, [&](unsigned id) { return targets_.contains(id); }, [&](unsigned id) {
    if (set_.verbose) std::cout << "Target(" << id << ") already exists!" << std::endl;
  });
  std::vector<std::vector<long>> rows(batches_.size());
  for (long i : keep) rows[(size_t)cls_batch[class_of[i]]].push_back(i);
  long created = 0;
  for (size_t b = 0; b < rows.size(); ++b) {
    const long k = (long)rows[b].size();
    if (!k) continue;
    const std::vector<unsigned> ids2 = gatherRows(ids, rows[b], 1);
    RowsIn<double> p2(p0, &rows[b], 7), v2(v0, &rows[b], 6), a2(a0, &rows[b], 6);
    std::vector<int> cls2((size_t)k), pidx((size_t)k);
    for (long j = 0; j < k; ++j) {
      const unsigned c = class_of[rows[b][(size_t)j]];
      cls2[(size_t)j] = cls_idx[c];
      pidx[(size_t)j] = (int)c;
    }
    const long first = batches_[b]->append(k, ids2.data(), t0, P0, false, p2.get(), v2.get(), a2.get(), 0, cls2.data(), pidx.data(), n_classes);
    targets_.reserve(targets_.size() + (size_t)k);
    for (long j = 0; j < k; ++j) targets_.set(ids2[(size_t)j], Loc{(int)b, (int)(first + j)});
    created += k;
  }
  dev_ids_.dirty = true;
  return created;
}

void Shard::updateAll(double dt) {
  for (auto& b : batches_) b->step_dense(dt, nullptr, 0, nullptr);
}

bool Shard::erase(unsigned id) {
  Loc loc;
  if (!find(id, loc)) {
    notFound(id);
    return false;
  }
  Batch* b = batches_[(size_t)loc.batch].get();
  const bool was_last = loc.slot == b->size() - 1;
  const unsigned moved = b->erase_slot(loc.slot);
  targets_.erase(id);
  dev_ids_.dirty = true;
  if (!was_last) targets_.set(moved, Loc{loc.batch, loc.slot});
  return true;
}

long Shard::eraseBatch(const unsigned* ids, long n, std::vector<unsigned>& erased) {
  std::vector<std::vector<int>> slots(batches_.size());
  long gone = 0;
  for (long i = 0; i < n; ++i) {
    Loc loc;
    if (!find(ids[i], loc)) {     // unknown, or already taken by an earlier entry of this call
      notFound(ids[i]);
      continue;
    }
    slots[(size_t)loc.batch].push_back(loc.slot);
    erased.push_back(ids[i]);
    targets_.erase(ids[i]);
    ++gone;
  }
  std::vector<std::pair<unsigned, int>> moves;
  dev_ids_.dirty = true;
  for (size_t b = 0; b < batches_.size(); ++b) {
    if (slots[b].empty()) continue;
    batches_[b]->erase_slots(slots[b].data(), (long)slots[b].size(), moves);
    for (auto const& mv : moves) targets_.set(mv.first, Loc{(int)b, mv.second});
  }
  return gone;
}

bool Shard::time(unsigned id, double& t) {
  Loc loc;
  if (!find(id, loc)) return false;
  t = batches_[(size_t)loc.batch]->time(loc.slot);
  return true;
}

int Shard::state(unsigned id, double* x, double* P) {
  Loc loc;
  if (!find(id, loc)) return 0;
  Batch* b = batches_[(size_t)loc.batch].get();
  b->get_state(&loc.slot, 1, x, P);
  return b->n_state();
}

long long Shard::numberMeasurements(unsigned id) {
  Loc loc;
  if (find(id, loc)) return batches_[(size_t)loc.batch]->n_measurements(loc.slot);
  notFound(id);
  return 0;
}

int Shard::rejectionRun(unsigned id) {
  Loc loc;
  if (find(id, loc)) return batches_[(size_t)loc.batch]->rejection_run(loc.slot);
  return -1;
}

bool Shard::trackCounts(unsigned id, int& miss, int& hits) {
  Loc loc;
  if (!find(id, loc)) return false;
  batches_[(size_t)loc.batch]->track_count(loc.slot, miss, hits);
  return true;
}

// Node-tick sizes (a few to a thousand targets per call) are a LATENCY path: staging copies and separate launches cost more than
// the step itself (40 targets: 22 us for the dense host path below, 78 us with the getters behind it).  They go through the
// one-target queue instead -- host table look-up per id, one indexed launch at the next read, the queue behind the PCIe BAR and the
// getter table filled by the same launch for up to a wavefront of targets (Batch::flush) -- as a caller looping over the
// reference's own symbols would, minus the call overhead.  Same results (tests/test_gpu_by_id.py, tests/test_gpu_ingest.py).
bool Shard::smallBatchPath(long n) const {
  if (n <= 0 || n > set_.small_batch_most) return false;
  for (const auto& b : batches_)
    if (!b->getter_table_is_cheap()) return false;   // (a batch too large for a host-resident getter table: the bulk paths below)
  return true;
}

namespace {
// the update policy's rows of a device-resolved call: -2 / 0 (an unknown id) everywhere ahead of the batches' launches, and -1
// ("no measurement judged") at the entries of a batch that steps without a policy
__global__ void gate_rows_fill_kernel(double* nis, unsigned char* ev, long n) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) { nis[e] = -2.0; ev[e] = 0; }
}
__global__ void gate_rows_unjudged_kernel(const int* idx, double* nis, long n) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n && idx[e] >= 0) nis[e] = -1.0;
}
}  // namespace

void Shard::updateGateChanged(int type) {
  for (auto& b : batches_)
    if (b->type() == type) b->set_update_gate(set_.gate[type]);
}

void Shard::checkUpdateGate(const unsigned* ids, long n) const {
  std::vector<const char*> why(batches_.size(), nullptr);
  bool any = false;
  for (size_t b = 0; b < batches_.size(); ++b) { why[b] = batches_[b]->update_gate_refusal(); any = any || why[b]; }
  if (!any) return;
  for (long i = 0; i < n; ++i) {
    Loc loc;
    if (find(ids[i], loc) && why[(size_t)loc.batch]) throw std::runtime_error(why[(size_t)loc.batch]);
  }
}

int Shard::updateGateServed(int type) const {
  int r = -1;
  for (const auto& b : batches_)
    if (b->type() == type) {
      const bool ok = b->update_gate_refusal(set_.gate[type].on() ? set_.gate[type] : UpdateGate{1.0, -1}) == nullptr;
      r = (r == 0 || !ok) ? 0 : 1;
    }
  return r;
}

long Shard::updateBatch(const unsigned* ids, long n, double dt, const double* meas, const unsigned char* has_meas, double* nis_out,
                        unsigned char* event_out) {
  const size_t nb = batches_.size();
  const bool outs = nis_out || event_out;
  if (nis_out) std::fill(nis_out, nis_out + (n > 0 ? n : 0), -2.0);
  if (event_out) std::fill(event_out, event_out + (n > 0 ? n : 0), (unsigned char)0);
  if (smallBatchPath(n)) {
    long done = 0;
    if (outs) for (auto& b : batches_) b->set_gate_sink(nis_out, event_out);
    try {
      for (long i = 0; i < n; ++i) {
        Loc loc;
        if (!find(ids[i], loc)) {
          if (set_.verbose) notFound(ids[i]);
          continue;
        }
        batches_[(size_t)loc.batch]->step_one(loc.slot, dt, (meas && (!has_meas || has_meas[i])) ? meas + 7 * i : nullptr, outs ? i : -1);
        ++done;
      }
      if (outs) for (auto& b : batches_) b->flush();   // the outputs are in the caller's arrays when the call returns
    } catch (...) {
      for (auto& b : batches_) b->set_gate_sink(nullptr, nullptr);
      throw;
    }
    if (outs) for (auto& b : batches_) b->set_gate_sink(nullptr, nullptr);
    return done;
  }
  if (Batch* bt = wholeBatch(ids, n)) {   // no per-id lookup, dense kernel
    bt->step_dense_host(dt, meas, has_meas, nis_out, event_out);
    return n;
  }
  // ids in any order, possibly several batches, possibly unknown ids: resolved on the device (id_resolve.hpp); a call
  // that names an id twice keeps the reference's "two consecutive steps" through the host path below
  if (n >= kDevResolveMin && !set_.verbose) {
    ResolveCounters rc;
    if (resolveOnDevice(ids, n, rc) && !rc.duplicate) {
      DevIds& d = dev_ids_;
      if (meas) {
        TE_HIP_CHECK(hipMemcpyAsync(d.aos.get(), meas, sizeof(double) * 7 * n, hipMemcpyHostToDevice, stream_));
        batches_[0]->pack_meas_dev(d.aos.get(), n, d.soa.get(), n);
      }
      if (meas && has_meas) TE_HIP_CHECK(hipMemcpyAsync(d.mask.get(), has_meas, (size_t)n, hipMemcpyHostToDevice, stream_));
      long total = 0;
      bool rows = outs;   // the policy's rows by entry: for the caller, or as the kernel's NIS row alone
      for (size_t b = 0; b < nb && !rows; ++b) rows = meas && rc.found[b] > 0 && batches_[b]->update_gate().on();
      if (rows) hipLaunchKernelGGL(gate_rows_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d.gnis.get(), d.gev.get(), n);
      for (size_t b = 0; b < nb; ++b) {
        if (rc.found[b] <= 0) continue;
        total += rc.found[b];
        hipLaunchKernelGGL(id_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d.loc.get(), n, (int)b, d.idx.get(),
                           (unsigned char*)nullptr);
        const bool pol = meas && batches_[b]->update_gate().on();
        if (rows && !pol) hipLaunchKernelGGL(gate_rows_unjudged_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d.idx.get(), d.gnis.get(), n);
        batches_[b]->step_indexed_dev(d.idx.get(), n, dt, meas ? d.soa.get() : nullptr, n, (meas && has_meas) ? d.mask.get() : nullptr, rows ? d.gnis.get() : nullptr,
                                      rows ? d.gev.get() : nullptr);
      }
      if (nis_out) TE_HIP_CHECK(hipMemcpyAsync(nis_out, d.gnis.get(), sizeof(double) * n, hipMemcpyDeviceToHost, stream_));
      if (event_out) TE_HIP_CHECK(hipMemcpyAsync(event_out, d.gev.get(), (size_t)n, hipMemcpyDeviceToHost, stream_));
      TE_HIP_CHECK(hipStreamSynchronize(stream_));   // the caller's host arrays may be reused after return
      return total;
    }
  }
  // The host path: the ids by batch, one indexed step per batch.  The same id twice in one call = two consecutive steps, as
  // the reference's loop over ids would do: everything queued so far for that batch goes first.
  std::vector<std::vector<unsigned char>> seen(nb);
  for (size_t b = 0; b < nb; ++b) seen[b].assign((size_t)batches_[b]->size(), 0);
  BySlot by;
  auto step = [&](size_t b, const std::vector<long>* pos) {   // (pos null: the caller's arrays are this batch's rows already)
    RowsIn<double> m2(meas, pos, 7);
    RowsIn<unsigned char> h2(has_meas, pos, 1);
    RowsOut<double> n2(nis_out, pos, 1);
    RowsOut<unsigned char> e2(event_out, pos, 1);
    batches_[b]->step_indexed(by.slots[b].data(), (long)by.slots[b].size(), dt, m2.get(), h2.get(), n2.get(), e2.get());
    scatterAll(n2, e2);
  };
  splitBySlot(ids, n, by, [&](size_t b, const Loc& loc) {
    if (seen[b][(size_t)loc.slot]) {
      step(b, &by.sp.src[b]);
      for (int s : by.slots[b]) seen[b][(size_t)s] = 0;
      by.slots[b].clear();
      by.sp.src[b].clear();
    }
    seen[b][(size_t)loc.slot] = 1;
  });
  if (set_.verbose) for (long i : by.sp.unknown) notFound(ids[i]);
  for (size_t b = 0; b < nb; ++b) {
    const long k = (long)by.slots[b].size();
    if (k) step(b, k == n ? nullptr : &by.sp.src[b]);   // k == n: single batch, every id known: rows already in order
  }
  return by.known;
}

long Shard::getPoseBatch(const unsigned* ids, long n, double* pose, double* twist, double* acc,
                                 unsigned char* found, bool at_time, double t1) {
  const size_t nb = batches_.size();
  if (!at_time && smallBatchPath(n)) {   // rows from the host-resident getter table (filled by the flush's own launch)
    long done = 0;
    for (long i = 0; i < n; ++i) {
      Loc loc;
      const bool ok = find(ids[i], loc);
      if (found) found[i] = ok ? 1 : 0;
      if (!ok) continue;
      batches_[(size_t)loc.batch]->outputs_one(loc.slot, pose ? pose + 7 * i : nullptr, twist ? twist + 6 * i : nullptr, acc ? acc + 6 * i : nullptr, false, 0.0);
      ++done;
    }
    return done;
  }
  if (Batch* bt = wholeBatch(ids, n)) {
    bt->outputs(nullptr, n, pose, twist, acc, at_time, t1);
    if (found) std::memset(found, 1, (size_t)n);
    return n;
  }
  if (n >= kDevResolveMin) {   // ids resolved on the device; rows come back in the caller's order
    ResolveCounters rc;
    if (resolveOnDevice(ids, n, rc)) {
      DevIds& d = dev_ids_;
      long total = 0;
      double* dp = pose ? d.out.get() : nullptr;
      double* dtw = twist ? d.out.get() + 7 * n : nullptr;
      double* da = acc ? d.out.get() + 13 * n : nullptr;
      for (size_t b = 0; b < nb; ++b) {
        if (rc.found[b] <= 0) continue;
        total += rc.found[b];
        hipLaunchKernelGGL(id_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d.loc.get(), n, (int)b, d.idx.get(),
                           (unsigned char*)nullptr);
        batches_[b]->outputs_indexed_dev(d.idx.get(), n, dp, dtw, da, at_time, t1);
      }
      if (total == n) {   // every id known: straight into the caller's arrays
        if (pose) TE_HIP_CHECK(hipMemcpyAsync(pose, dp, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, stream_));
        if (twist) TE_HIP_CHECK(hipMemcpyAsync(twist, dtw, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, stream_));
        if (acc) TE_HIP_CHECK(hipMemcpyAsync(acc, da, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, stream_));
        TE_HIP_CHECK(hipStreamSynchronize(stream_));
        if (found) std::memset(found, 1, (size_t)n);
      } else {            // rows of unknown ids stay as the caller left them
        std::vector<double> hp(pose ? (size_t)n * 7 : 0), ht(twist ? (size_t)n * 6 : 0), ha(acc ? (size_t)n * 6 : 0);
        std::vector<int> hloc((size_t)n);
        if (pose) TE_HIP_CHECK(hipMemcpyAsync(hp.data(), dp, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, stream_));
        if (twist) TE_HIP_CHECK(hipMemcpyAsync(ht.data(), dtw, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, stream_));
        if (acc) TE_HIP_CHECK(hipMemcpyAsync(ha.data(), da, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, stream_));
        TE_HIP_CHECK(hipMemcpyAsync(hloc.data(), d.loc.get(), sizeof(int) * n, hipMemcpyDeviceToHost, stream_));
        TE_HIP_CHECK(hipStreamSynchronize(stream_));
        for (long i = 0; i < n; ++i) {
          const bool ok = hloc[(size_t)i] >= 0;
          if (found) found[i] = ok ? 1 : 0;
          if (!ok) continue;
          if (pose) std::memcpy(pose + i * 7, &hp[(size_t)i * 7], sizeof(double) * 7);
          if (twist) std::memcpy(twist + i * 6, &ht[(size_t)i * 6], sizeof(double) * 6);
          if (acc) std::memcpy(acc + i * 6, &ha[(size_t)i * 6], sizeof(double) * 6);
        }
      }
      return total;
    }
  }
  BySlot by;
  splitBySlot(ids, n, by, [](size_t, const Loc&) {});
  mark_found(found, n, by.sp.unknown);
  for (size_t b = 0; b < nb; ++b) {
    const long k = (long)by.slots[b].size();
    if (!k) continue;
    const std::vector<long>* pos = k == n ? nullptr : &by.sp.src[b];   // k == n: straight into the caller's arrays
    RowsOut<double> p2(pose, pos, 7), t2(twist, pos, 6), a2(acc, pos, 6);
    batches_[b]->outputs(by.slots[b].data(), k, p2.get(), t2.get(), a2.get(), at_time, t1);
    scatterAll(p2, t2, a2);
  }
  return by.known;
}

long Shard::getStateBatch(const unsigned* ids, long n, double* x, double* P) {
  std::vector<int> slots((size_t)n);
  int b0 = -1;
  for (long i = 0; i < n; ++i) {
    Loc loc;
    if (!find(ids[i], loc)) return -1;
    if (b0 < 0) b0 = loc.batch;
    if (loc.batch != b0) return -2;  // all ids must belong to one batch (one state size)
    slots[(size_t)i] = loc.slot;
  }
  batches_[(size_t)b0]->get_state(slots.data(), n, x, P);
  return batches_[(size_t)b0]->n_state();
}

double Shard::intersectTime(unsigned id, double t1, const double* origin, double radius) {
  Loc loc;
  if (!find(id, loc)) return -1;
  double d = -1;
  batches_[(size_t)loc.batch]->intersect(&loc.slot, 1, t1, origin, radius, &d, nullptr);
  return d;
}

bool Shard::intersectPose(unsigned id, double t1, const double* origin, double radius, double* pose7, double* delta) {
  pose7[0] = pose7[1] = pose7[2] = pose7[3] = pose7[4] = pose7[5] = 0.0;
  pose7[6] = 1.0;  // initPose, intersection_solver.cpp:99
  if (delta) *delta = -1;
  Loc loc;
  if (!find(id, loc)) return false;
  double d = -1;
  batches_[(size_t)loc.batch]->intersect(&loc.slot, 1, t1, origin, radius, &d, pose7);
  if (delta) *delta = d;
  return d > -1;
}

long Shard::intersectGatedBatch(const unsigned* ids, long n, double t1, double pos_th, double ang_th, const double* origin, double radius,
                                double* delta, double* pose, unsigned char* converged, unsigned char* found, double* filt) {
  for (long i = 0; i < n; ++i) no_intersection(i, delta, pose, converged, filt);
  BySlot by;
  splitBySlot(ids, n, by, [](size_t, const Loc&) {});
  mark_found(found, n, by.sp.unknown);
  for (size_t b = 0; b < batches_.size(); ++b) {
    const long k = (long)by.slots[b].size();
    if (!k) continue;
    std::vector<double> d2((size_t)k), p2((size_t)k * 7), f2(filt ? (size_t)k * 2 : 0);
    std::vector<unsigned char> c2((size_t)k);
    batches_[b]->intersect_gated(by.slots[b].data(), k, t1, origin, radius, pos_th, ang_th, set_.filters_length, d2.data(), p2.data(), c2.data(),
                                 filt ? f2.data() : nullptr);
    scatterRows(delta, d2, by.sp.src[b], 1);
    scatterRows(converged, c2, by.sp.src[b], 1);
    scatterRows(pose, p2, by.sp.src[b], 7);
    scatterRows(filt, f2, by.sp.src[b], 2);
  }
  return by.known;
}

long Shard::intersectBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, double* delta, double* pose,
                           unsigned char* found) {
  for (long i = 0; i < n; ++i) no_intersection(i, delta, pose, nullptr, nullptr);
  BySlot by;
  splitBySlot(ids, n, by, [](size_t, const Loc&) {});
  mark_found(found, n, by.sp.unknown);
  for (size_t b = 0; b < batches_.size(); ++b) {
    const long k = (long)by.slots[b].size();
    if (!k) continue;
    std::vector<double> d2((size_t)k), p2(pose ? (size_t)k * 7 : 0);
    batches_[b]->intersect(by.slots[b].data(), k, t1, origin, radius, d2.data(), pose ? p2.data() : nullptr);
    scatterRows(delta, d2, by.sp.src[b], 1);
    scatterRows(pose, p2, by.sp.src[b], 7);
  }
  return by.known;
}

Batch* Shard::batchOfType(int type) {
  for (auto& b : batches_)
    if (b->type() == type) return b.get();
  return nullptr;
}

long Shard::rows() const {
  long rows = 0;
  for (auto& b : batches_) rows += b->size();
  return rows;
}

void Shard::posesToDevice(double* out_dev) {
  long off = 0;
  for (auto& b : batches_) {
    if (!b->size()) continue;
    b->outputs_dev(out_dev + off * 7, nullptr, nullptr, false, 0.0);
    off += b->size();
  }
}

void Shard::setStream(hipStream_t s) {
  for (auto& b : batches_) { b->synchronize(); b->set_stream(s); }
  stream_ = s;
}

// Can the tick of all batches be ONE launch?  At least two non-empty batches, every one of them a one-class batch in the
// separable layout with packed groups (the automatic choice for the shipped models) -- then there is at most one batch per motion
// model.  ShardSettings::population_tick off (TE_POPULATION_TICK=0) keeps the launch per batch (experiments, and the comparison in profiles/).
bool Shard::populationTick() const {
  if (!set_.population_tick) return false;
  int present = 0, shared = 0;
  bool seen[4] = {false, false, false, false};
  for (const auto& b : batches_) {
    if (b->size() == 0) continue;
    if (!b->population_ready() || b->type() < 0 || b->type() > 3 || seen[b->type()]) return false;
    seen[b->type()] = true;
    ++present;
    shared += b->shared_axes() ? 1 : 0;
  }
  return present >= 2 && (shared == 0 || shared == present);   // (one kernel steps all parts: all in the shared-axes form, or none)
}

void Shard::enqueuePopulationTick(hipStream_t st, long s, double dt, const Batch::SeqSpec* specs, bool query, const double* origin,
                                          double radius, bool reverse, bool ab) {
  StepParams parts[4];
  for (auto& q : parts) { q = StepParams{}; q.n = 0; q.idx = nullptr; }
  Batch* swap[4] = {nullptr, nullptr, nullptr, nullptr};
  // An innovation stream on any batch: the tick is the INNOV population kernel -- a plain tick in place -- and what that kernel
  // does not carry follows per batch as the launches that exist for it: the pose writer, intersect_kernel (same results).
  bool innov = false;
  for (size_t b = 0; b < batches_.size(); ++b) innov = innov || (batches_[b]->size() > 0 && specs[b].innov.on());
  if (innov) {
    bool shared_form = false;
    for (size_t b = 0; b < batches_.size(); ++b) {
      if (batches_[b]->size() == 0) continue;
      const int t = batches_[b]->type();
      parts[t] = batches_[b]->tick_params(s, dt, specs[b], false, origin, radius, false);
      parts[t].pose = nullptr;
      shared_form = batches_[b]->shared_axes();
    }
    launch_population_step(set_.dtype, parts, false, false, reverse, st, shared_form);
    for (size_t b = 0; b < batches_.size(); ++b) batches_[b]->enqueue_after_innov_tick(st, s, specs[b], query, origin, radius);
    return;
  }
  bool ab_all = ab, shared = false;
  for (int pass = 0; pass < 2; ++pass) {   // (a batch without room for its second record buffer puts the whole tick in place)
    for (size_t b = 0; b < batches_.size(); ++b) {
      if (batches_[b]->size() == 0) continue;
      const int t = batches_[b]->type();
      parts[t] = batches_[b]->tick_params(s, dt, specs[b], query, origin, radius, ab_all);
      if (ab_all && !parts[t].rec_out) { ab_all = false; break; }
      swap[t] = batches_[b].get();
      shared = batches_[b]->shared_axes();   // (populationTick: the same for every non-empty batch)
    }
    if (ab_all == ab || pass == 1) break;
  }
  if (!ab_all) for (auto& q : parts) q.rec_out = nullptr;
  launch_population_step(set_.dtype, parts, query, ab_all, reverse, st, shared);
  if (ab_all) for (auto* b : swap) if (b) b->swap_records();
}

void Shard::stepSequenceAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, bool query,
                                    const double* origin, double radius, int use_graph, const DtSchedule& sched) {
  const size_t nb = batches_.size();
  if ((size_t)n_specs != nb) throw std::runtime_error("target_estimation_amd: stepSequenceAll needs one spec per batch");
  if (sched.on() && sched.n != n_ticks) throw std::invalid_argument("target_estimation_amd: the time-step schedule has one entry per tick of the call");
  for (size_t b = 0; b < nb; ++b) {   // (before anything is enqueued)
    batches_[b]->check_pose_stream(specs[b].poses);
    batches_[b]->check_innov_stream(specs[b].innov);
  }
  if (n_ticks <= 0 || nb == 0) return;
  if (query && !origin) throw std::runtime_error("target_estimation_amd: stepSequenceAll: query without an origin");
  for (size_t b = 0; b < nb; ++b) {
    if (query && batches_[b]->size() > 0 && !specs[b].delta_dev)
      throw std::runtime_error("target_estimation_amd: stepSequenceAll: query without a delta output");
    batches_[b]->prepare();   // queued one-target steps run first
    batches_[b]->prepare_reacquire(specs[b].innov);   // (the device tables of a re-acquisition policy, before anything is recorded)
  }
  const double zero3[3] = {0, 0, 0};
  const double* org = origin ? origin : zero3;
  if (!use_graph) {
    // Zig-zag over the WHOLE tick: tick s walks batch 0 .. nb-1, tiles forwards; tick s+1 walks batch nb-1 .. 0, tiles
    // backwards, so that what the Infinity Cache still holds at the end of a tick is what the next tick reads first.
    long state = 0;
    for (size_t b = 0; b < nb; ++b) state += batches_[b]->state_bytes();
    // (backwards = the workgroups mirrored inside each class b % 8, zigzag_map.hpp: a tile keeps its XCD both ways.  The
    // threshold dates from the plain mirror, which moved L2-resident populations' tiles to another XCD; not measured again.)
    const bool zz = state >= Batch::zigzag_min_bytes();
    // A -> B ticks (Batch::pingpong_min_bytes) by the size of the WHOLE population: what decides is how much is streamed
    // between two uses of a record, not which batch it belongs to
    const bool ab = Batch::pingpong_min_bytes() >= 0 && state >= Batch::pingpong_min_bytes();
    const bool pop = populationTick();
    for (long s = 0; s < n_ticks; ++s) {
      const bool rev = zz && seq_flip_;
      if (pop) {
        enqueuePopulationTick(stream_, s, sched.at(s, dt), specs, query, org, radius, rev, ab && !query);
      } else {
        for (size_t k = 0; k < nb; ++k) {
          const size_t b = rev ? nb - 1 - k : k;
          batches_[b]->enqueue_tick(stream_, s, sched.at(s, dt), specs[b], query, org, radius, rev, ab);
        }
      }
      seq_flip_ = !seq_flip_;
    }
    TE_HIP_CHECK(hipGetLastError());
  } else {
    auto* hit = seq_graphs_.find([&](const SeqKey& g) {
      if (g.n_ticks != n_ticks || !g.dt.matches(sched, dt) || g.query != query || g.specs.size() != nb) return false;
      if (query && (g.origin[0] != org[0] || g.origin[1] != org[1] || g.origin[2] != org[2] || g.radius != radius)) return false;
      for (size_t b = 0; b < nb; ++b)
        if (!g.specs[b].same(specs[b]) || !g.ident[b].same(batches_[b]->dev_identity())) return false;
      return true;
    });
    if (!hit) {
      if (branch_streams_.empty()) {
        Stream st; TE_HIP_CHECK(hipStreamCreateWithFlags(st.out(), hipStreamNonBlocking));
        branch_streams_.push_back(std::move(st));
      }
      SeqKey key{n_ticks, DtKey(sched, dt), query, {org[0], org[1], org[2]}, radius, std::vector<Batch::SeqSpec>(specs, specs + nb), {}};
      for (size_t b = 0; b < nb; ++b) key.ident.push_back(batches_[b]->dev_identity());
      // The launches are captured on ONE stream whose dependency set is replaced at the head of every
      // batch's chain (hipStreamUpdateCaptureDependencies): the chains become the branches of the graph.
      hipStream_t cap = branch_streams_[0].get();
      using Nodes = std::vector<hipGraphNode_t>;
      auto set_deps = [&](Nodes& deps) {
        TE_HIP_CHECK(hipStreamUpdateCaptureDependencies(cap, deps.empty() ? nullptr : deps.data(), deps.size(), hipStreamSetCaptureDependencies));
      };
      auto captured = [&]() {   // the node(s) the next launch would depend on = what was just captured
        hipStreamCaptureStatus status; unsigned long long id = 0; hipGraph_t gr = nullptr;
        const hipGraphNode_t* deps = nullptr; size_t n = 0;
        TE_HIP_CHECK(hipStreamGetCaptureInfo_v2(cap, &status, &id, &gr, &deps, &n));
        return Nodes(deps, deps + n);
      };
      hit = &seq_graphs_.record(std::move(key), stream_, cap, [&] {
        std::deque<Batch::RecordingScope> recording;   // (uniform tiles: a recording's ticks promote)
        for (size_t b = 0; b < nb; ++b) recording.emplace_back(*batches_[b]);
        Nodes leaves, none;
        if (populationTick()) {
          // one launch per tick for the whole population: a single chain, nothing left to the placement of branches on
          // hardware queues (kf_step_sep.hpp, kf_step_population_kernel)
          long state = 0;
          for (size_t b = 0; b < nb; ++b) state += batches_[b]->state_bytes();
          const bool zz = state >= Batch::zigzag_min_bytes();
          for (long s = 0; s < n_ticks; ++s) enqueuePopulationTick(cap, s, sched.at(s, dt), specs, query, org, radius, zz && (s & 1) != 0, false);
        } else
        for (size_t b = 0; b < nb; ++b) {
          if (batches_[b]->size() == 0) continue;
          set_deps(none);                                  // a new chain: no predecessor
          const bool zz = batches_[b]->state_bytes() >= Batch::zigzag_min_bytes();
          for (long s = 0; s < n_ticks; ++s) batches_[b]->enqueue_tick(cap, s, sched.at(s, dt), specs[b], query, org, radius, zz && (s & 1) != 0);
#ifdef TE_TEST_HOOKS   // only in libtarget_estimation_amd_testhooks.so (csrc/Makefile `testhooks`), never in the product library
          if (std::getenv("TE_TEST_FAIL_IN_CAPTURE")) throw std::runtime_error("target_estimation_amd: injected failure inside stream capture");
#endif
          const Nodes tail = captured();
          leaves.insert(leaves.end(), tail.begin(), tail.end());
        }
        TE_HIP_CHECK(hipGetLastError());
        if (!leaves.empty()) set_deps(leaves);
      });
    }
    if (use_graph == 2) return;
    TE_HIP_CHECK(hipGraphLaunch(hit->exec.get(), stream_));
    for (size_t b = 0; b < nb; ++b) batches_[b]->note_replay(n_ticks);
  }
  for (size_t b = 0; b < nb; ++b) {
    if (batches_[b]->size() == 0) continue;
    batches_[b]->account(n_ticks, dt, sched, specs[b].all_measured());
  }
}

// The route of a fused replay of all batches (step_variant.hpp, plan_fused_all), from the batches as they are and the call's streams
FusedAllRoute Shard::fusedAllRoute(const Batch::SeqSpec* specs, bool scheduled, long n_ticks) const {
  std::vector<FusedAllBatch> fb(batches_.size());
  for (size_t b = 0; b < batches_.size(); ++b) {
    const Batch& q = *batches_[b];
    FusedAllBatch& f = fb[b];
    f.n = q.size(); f.type = q.type(); f.ready = q.population_ready(); f.keep_meas = q.keep_measurement();
    if (!specs) continue;   // (a question about the batches alone: fusedAllServed)
    f.pose = specs[b].poses.dev != nullptr;
    f.nis = specs[b].innov.on();
    f.gate_or_policy = specs[b].innov.gated() || specs[b].innov.reacq.on;
  }
  return plan_fused_all(set_.population_tick, set_.dtype == F64, fb.data(), (long)fb.size(), scheduled, n_ticks, kDtTabMaxTicks);
}

int Shard::fusedAllServed(bool gated, bool scheduled) const {
  std::vector<Batch::SeqSpec> specs(batches_.size(), Batch::SeqSpec{nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 0});
  static double some_row;   // (never dereferenced: the route asks whether a batch carries rows, not where)
  if (gated) for (auto& q : specs) { q.innov.nis = &some_row; q.innov.gate = 1.0; }
  return fusedAllRoute(specs.data(), scheduled, 1) != FusedAllRoute::kPerBatch ? 1 : 0;
}

void Shard::stepFusedAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, const DtSchedule& sched) {
  const size_t nb = batches_.size();
  if ((size_t)n_specs != nb) throw std::runtime_error("target_estimation_amd: stepFusedAll needs one spec per batch");
  const FusedAllRoute route = fusedAllRoute(specs, sched.on(), n_ticks);
  for (size_t b = 0; b < nb; ++b) {   // every refusal of every batch's own call, before anything is enqueued or changed
    if (specs[b].ring_ticks != 0) throw std::invalid_argument("target_estimation_amd: stepFusedAll: a fused call reads its measurements linearly (ring_ticks must be 0)");
    batches_[b]->check_fused_call(n_ticks, specs[b], sched, route != FusedAllRoute::kPerBatch || batches_[b]->fused_call_one_launch(specs[b], sched));
  }
  if (nb == 0) return;
  if (route == FusedAllRoute::kPerBatch) {   // the per-batch calls in batch order: same bits, their launch counts
    for (size_t b = 0; b < nb; ++b)
      batches_[b]->step_fused_gated(n_ticks, dt, specs[b].meas_base, specs[b].tick_stride, specs[b].ld, specs[b].has_base, specs[b].has_stride,
                                    specs[b].poses, specs[b].innov, sched);
    return;
  }
  for (size_t b = 0; b < nb; ++b) batches_[b]->fused_call_begin(specs[b]);
  if (n_ticks <= 0) return;
  // one table for all parts: a run of the shard's ring that no other call shares, filled on the stream ahead of the launch
  const double* dt_tab = sched.on() ? dttab_.push(sched.dt, n_ticks, stream_) : nullptr;
  StepParams parts[4];
  for (auto& q : parts) { q = StepParams{}; q.n = 0; }
  for (size_t b = 0; b < nb; ++b)
    if (batches_[b]->size() > 0) parts[batches_[b]->type()] = batches_[b]->fused_call_params(n_ticks, dt, specs[b], sched, dt_tab);
  launch_population_fused(set_.dtype, parts, route == FusedAllRoute::kGatedLoop, dt_tab, stream_);
  TE_HIP_CHECK(hipGetLastError());
  for (size_t b = 0; b < nb; ++b)
    if (batches_[b]->size() > 0) batches_[b]->account(n_ticks, dt, sched, specs[b].all_measured());
}

void Shard::liveStartAll(double dt, const Batch::SeqSpec* specs, long n_specs, long first_entry, long max_ticks, double idle_limit_s,
                         bool query, const double* origin, double radius) {
  const size_t nb = batches_.size();
  if ((size_t)n_specs != nb || nb == 0) throw std::runtime_error("target_estimation_amd: liveStartAll needs one spec per batch");
  if (query && !origin) throw std::runtime_error("target_estimation_amd: liveStartAll: query without an origin");
  for (size_t b = 0; b < nb; ++b)
    if (query && !specs[b].delta_dev) throw std::runtime_error("target_estimation_amd: liveStartAll: query without a delta output");
  double share = 0.0;
  for (size_t b = 0; b < nb; ++b) {
    if (batches_[b]->size() == 0) throw std::runtime_error("target_estimation_amd: liveStartAll: an empty batch");
    if (specs[b].ring_ticks <= 0) throw std::invalid_argument("target_estimation_amd: liveStartAll: every batch needs a measurement ring");
    const long cap = batches_[b]->live_capacity_next(query);   // (of the kernel this batch's session runs: plain, with outputs, or gated)
    if (cap <= 0) throw std::runtime_error("target_estimation_amd: live mode needs the axis-separable layout with packed groups (batch " + std::to_string(b) + ")");
    share += (double)(batches_[b]->size() + batches_[b]->layout().tpw) / (double)cap;   // + one tile for the relay wavefront
  }
  if (share > 1.0)
    throw std::runtime_error("target_estimation_amd: liveStartAll: the batches' resident kernels do not fit the device together (" +
                             std::to_string(share) + " of its capacity)");
  size_t started = 0;
  try {
    for (; started < nb; ++started)
      batches_[started]->live_start(dt, specs[started].meas_base, specs[started].tick_stride, specs[started].ld, specs[started].has_base,
                                    specs[started].has_stride, specs[started].ring_ticks, first_entry, max_ticks, idle_limit_s,
                                    query ? origin : nullptr, radius, query ? specs[started].delta_dev : nullptr,
                                    query ? specs[started].pose_dev : nullptr);
    // side by side, or not at all: a kernel that could only start because an earlier one gave up (one hardware queue for all
    // of them and an idle limit shorter than the start timeout) is not a session
    for (size_t b = 0; b < nb; ++b)
      if (!batches_[b]->live_running())
        throw std::runtime_error("target_estimation_amd: liveStartAll: the batches' resident kernels do not run side by side (batch " + std::to_string(b) +
                                 " has ended already: they share a hardware queue -- more live batches than GPU_MAX_HW_QUEUES?)");
  } catch (...) {
    for (size_t b = 0; b < started; ++b) { try { batches_[b]->live_stop(); } catch (...) {} }
    throw;
  }
}

void Shard::livePostAll(long n_ticks, bool one_doorbell_per_tick) {
  if (one_doorbell_per_tick) {
    for (long i = 0; i < n_ticks; ++i)
      for (auto& b : batches_) b->live_post(1);
  } else {
    for (auto& b : batches_) b->live_post(n_ticks);
  }
}

long Shard::liveDoneAll() {
  long mn = -1;
  for (auto& b : batches_) {
    if (!b->live_active()) continue;
    const long d = b->live_done();
    mn = mn < 0 ? d : std::min(mn, d);
  }
  return mn < 0 ? 0 : mn;
}

std::vector<Batch*> Shard::liveOpenBatches() {
  std::vector<Batch*> open;
  for (auto& b : batches_) if (b->live_active()) open.push_back(b.get());
  return open;
}

long Shard::liveStopAll() {
  long served = -1;
  std::string err;
  for (auto& b : batches_) {
    if (!b->live_active()) continue;
    try {
      const long k = b->live_stop();
      if (served >= 0 && k != served) err = "target_estimation_amd: liveStopAll: the batches served different numbers of ticks";
      served = k;
    } catch (const std::exception& e) {
      err = e.what();
    }
  }
  if (!err.empty()) throw std::runtime_error(err);
  return served < 0 ? 0 : served;
}

void Shard::synchronize() {
  for (auto& b : batches_) b->synchronize();
}

void Shard::uploadRanks(const std::vector<unsigned>& sorted_all) {
  if (rank_maps_.size() < batches_.size()) rank_maps_.resize(batches_.size());
  for (size_t b = 0; b < batches_.size(); ++b) {
    const long n = batches_[b]->size();
    if (!n) continue;
    RankMap& r = rank_maps_[b];
    const hipStream_t st = batches_[b]->stream();
    if (r.cap < n) {   // a map that grows: the launches and the upload that still read the old buffers finish first
      const long want = std::max(n, r.cap * 2);
      TE_HIP_CHECK(hipStreamSynchronize(st));
      r.cap = 0;
      r.dev.reset(); r.host.reset();
      r.dev.alloc((size_t)want);
      r.host.alloc((size_t)want);
      if (!r.copied) TE_HIP_CHECK(hipEventCreateWithFlags(r.copied.out(), hipEventDisableTiming));
      r.cap = want;
    } else {
      TE_HIP_CHECK(hipEventSynchronize(r.copied.get()));   // the previous upload has left the staging buffer (long since, as a rule)
    }
    ranks_of_slots(sorted_all, batches_[b]->slot_ids().data(), n, r.host.host());
    TE_HIP_CHECK(hipMemcpyAsync(r.dev.get(), r.host.host(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));   // stream-ordered, no host wait
    TE_HIP_CHECK(hipEventRecord(r.copied.get(), st));
  }
}

// ---------------------------------------------------------------- the k soonest crossings (select_soonest.hpp)
void Shard::checkSelectSoonest(const SoonestSpec* specs, long n_specs, bool with_pose) const {
  const std::string pre = "target_estimation_amd: select_soonest: ";
  if (n_specs != (long)batches_.size()) throw std::invalid_argument(pre + "one description per batch is needed");
  long selected = 0;
  for (long b = 0; b < n_specs; ++b) {
    if (!specs[b].delta) continue;
    ++selected;
    if (with_pose && !specs[b].pose) throw std::invalid_argument(pre + "pose_out without pose_dev in batch " + std::to_string(b) + ": there is nothing to gather from");
  }
  check_soonest_parts(selected);
}

int Shard::soonestParts(const SoonestSpec* specs, long n_specs, int first_batch, SoonestPart* parts) const {
  int n = 0;
  for (long b = 0; b < n_specs; ++b)
    if (specs[b].delta) parts[n++] = SoonestPart{specs[b].delta, specs[b].ok, specs[b].pose, batches_[(size_t)b]->size(), first_batch + (int)b};
  return n;
}

void Shard::selectSoonestDev(const SoonestSpec* specs, long n_specs, int first_batch, double lo, double hi, int k, const SoonestOut& out) {
  checkSelectSoonest(specs, n_specs, out.pose != nullptr);
  SoonestPart parts[kSoonestMaxParts];
  const int n = soonestParts(specs, n_specs, first_batch, parts);
  soonest_.ensure(set_.soonest_max_wgs);
  launch_select_soonest(parts, n, lo, hi, k, out, soonest_, stream_);
}

void Shard::selectSoonestBegin(const SoonestSpec* specs, long n_specs, int first_batch, double lo, double hi, int k, bool with_pose) {
  checkSelectSoonest(specs, n_specs, with_pose);
  SoonestPart parts[kSoonestMaxParts];
  const int n = soonestParts(specs, n_specs, first_batch, parts);
  soonest_.ensure(set_.soonest_max_wgs);
  select_soonest_begin(parts, n, lo, hi, k, with_pose, soonest_, stream_);
}

long Shard::selectSoonestEnd(int k, bool with_pose, SoonestRow* rows) { return select_soonest_end(k, with_pose, soonest_, stream_, rows); }

// ---------------------------------------------------------------- covariance and time spread at a crossing (crossing_cov.hpp)
void Shard::crossingCovDev(double t1, const double* origin, double radius, const int* batch_dev, const int* slots_dev, const double* delta_dev,
                           long n, double sigma_r_max, double sigma_t_max, double* cov_dev, double* sigma_dev,
                           unsigned char* ok_dev) {
  check_crossing_cov_args(delta_dev != nullptr, origin != nullptr, radius, cov_dev != nullptr, sigma_dev != nullptr, ok_dev != nullptr,
                          sigma_r_max, sigma_t_max, true, n, 0);
  if (!batch_dev || !slots_dev) throw std::invalid_argument("target_estimation_amd: crossing_cov: the batch and slot lists are required");
  if (n == 0) return;
  launch_crossing_cov_orphans(batch_dev, n, (int)batches_.size(), cov_dev, sigma_dev, ok_dev, stream_);
  TE_HIP_CHECK(hipGetLastError());
  for (size_t b = 0; b < batches_.size(); ++b)
    batches_[b]->crossing_cov_dev(t1, origin, radius, delta_dev, slots_dev, n, sigma_r_max, sigma_t_max, cov_dev, sigma_dev, ok_dev, batch_dev, (int)b);
}

long Shard::crossingCovBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, const double* delta,
                             double sigma_r_max, double sigma_t_max, double* cov, double* sigma, unsigned char* ok) {
  check_crossing_cov_args(delta != nullptr, origin != nullptr, radius, cov != nullptr, sigma != nullptr, ok != nullptr, sigma_r_max,
                          sigma_t_max, false, 0, 0);
  for (long i = 0; i < n; ++i) crossing_cov_fill(i, cov, sigma, ok);
  BySlot by;
  splitBySlot(ids, n, by, [](size_t, const Loc&) {});
  for (size_t b = 0; b < batches_.size(); ++b) {
    const long k = (long)by.slots[b].size();
    if (!k) continue;
    const std::vector<double> d2 = gatherRows(delta, by.sp.src[b], 1);
    std::vector<double> c2((size_t)k * 6), s2(sigma ? (size_t)k * 2 : 0);
    std::vector<unsigned char> o2(ok ? (size_t)k : 0);
    batches_[b]->crossing_cov(by.slots[b].data(), k, t1, origin, radius, d2.data(), sigma_r_max, sigma_t_max, c2.data(),
                              sigma ? s2.data() : nullptr, ok ? o2.data() : nullptr);
    scatterRows(cov, c2, by.sp.src[b], 6);
    scatterRows(sigma, s2, by.sp.src[b], 2);
    scatterRows(ok, o2, by.sp.src[b], 1);
  }
  return by.known;
}

// ---------------------------------------------------------------- association of unlabelled detections (associate.hpp)
namespace {
void check_assoc_outs(const std::vector<std::unique_ptr<Batch>>& batches, const AssocSlotOut* out, long n_out, bool required) {
  const std::string pre = "target_estimation_amd: associate: ";
  if (n_out != (long)batches.size() || (n_out > 0 && !out)) throw std::invalid_argument(pre + "one output description per batch is needed");
  for (size_t b = 0; b < batches.size(); ++b) {
    if (required && (!out[b].meas || !out[b].has_meas)) throw std::invalid_argument(pre + "a required output is NULL");
    if (out[b].meas && out[b].ld < batches[b]->size())
      throw std::invalid_argument(pre + "ld " + std::to_string(out[b].ld) + " < size " + std::to_string(batches[b]->size()));
  }
}
}  // namespace

void Shard::associateDev(double dt, const double* det_dev, long M, double gate, long rounds, const AssocSlotOut* out, long n_out,
                         int* slot_of_det_dev, int* batch_of_det_dev, double* d2_of_det_dev, int* info_dev, double grid_cell) {
  check_assoc_args_for(grid_cell, dt, det_dev != nullptr, M, gate, rounds, info_dev != nullptr, 0, 0);
  check_assoc_outs(batches_, out, n_out, true);
  std::vector<Batch*> bs;
  for (auto& b : batches_) bs.push_back(b.get());
  associate_batches(bs.data(), (int)bs.size(), assoc_, set_.assoc_col_chunks, dt, det_dev, M, gate, rounds, out, slot_of_det_dev, batch_of_det_dev,
                    d2_of_det_dev, info_dev, stream_, grid_cell, set_.assoc_grid_buckets);
}

long Shard::associate(double dt, const double* det, long M, double gate, long rounds, const AssocSlotOut* out, long n_out, unsigned* ids_of_det,
                      int* batch_of_det, int* slot_of_det, double* d2_of_det, long* unmatched, long* n_unmatched, int* info, double grid_cell) {
  check_assoc_args_for(grid_cell, dt, det != nullptr, M, gate, rounds, true, 0, 0);
  std::vector<AssocSlotOut> none(batches_.size());
  if (!out) { out = none.data(); n_out = (long)none.size(); }   // (the host form's device outputs are optional)
  check_assoc_outs(batches_, out, n_out, false);
  std::vector<Batch*> bs;
  for (auto& b : batches_) bs.push_back(b.get());
  return associate_batches_host(bs.data(), (int)bs.size(), assoc_, set_.assoc_col_chunks, dt, det, M, gate, rounds, out, ids_of_det, batch_of_det,
                                slot_of_det, d2_of_det, unmatched, n_unmatched, info, stream_, grid_cell, set_.assoc_grid_buckets);
}

// ---------------------------------------------------------------- track lifecycle (lifecycle.hpp lists the launches)
void Shard::lifecycle(const double* det_dev, const int* slot_of_det_dev, long M, const unsigned char* const* has_dev, long n_masks,
                      const LifecyclePolicy& p, unsigned* retired_ids_out, long retired_cap, long* info) {
  const std::string pre = "target_estimation_amd: lifecycle: ";
  const long nb = (long)batches_.size();
  if (n_masks != nb) throw std::invalid_argument(pre + "n_batches " + std::to_string(n_masks) + " is not the manager's " + std::to_string(nb));
  long rows = 0;
  for (long b = 0; b < nb; ++b) {
    if (batches_[(size_t)b]->size() > 0 && !has_dev[b]) throw std::invalid_argument(pre + "the mask of a non-empty batch is NULL");
    rows += batches_[(size_t)b]->size();
  }
  const bool births = p.births() && M > 0;
  for (auto& b : batches_) b->prepare();   // the queued one-target steps and inits run first
  LifecycleScratch& s = life_;
  s.ensure(rows, M, nb);

  // THE PLAN, into the scratch alone
  long off = 0;
  for (long b = 0; b < nb; ++b) {
    Batch& bt = *batches_[(size_t)b];
    const long n = bt.size();
    if (n > 0) launch_lifecycle_count(has_dev[b], bt.track_miss_dev(), bt.track_hits_dev(), s.new_miss.get() + off, s.new_hits.get() + off,
                                      s.flag.get() + off, n, p.max_misses, stream_);
    launch_lifecycle_compact(s.flag.get() + off, 1, n, s.sums.get(), s.list.get() + off, s.counts.get() + b, stream_);
    off += n;
  }
  if (births) launch_lifecycle_det_flags(det_dev, slot_of_det_dev, s.flag.get() + rows, M, stream_);
  launch_lifecycle_compact(s.flag.get() + rows, kLifecycleDetCandidate, births ? M : 0, s.sums.get(), s.list.get() + rows, s.counts.get() + nb, stream_);
  launch_lifecycle_compact(s.flag.get() + rows, kLifecycleDetNonFinite, births ? M : 0, s.sums.get(), nullptr, s.counts.get() + nb + 1, stream_);
  int* h = s.host.host();
  TE_HIP_CHECK(hipMemcpyAsync(h, s.counts.get(), sizeof(int) * (size_t)(nb + 2), hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  long retired = 0;
  std::vector<long> stale_off((size_t)nb + 1, 0);   // where batch b's list lies behind the counts in the pinned block
  for (long b = 0; b < nb; ++b) {
    if (h[b] < 0 || h[b] > batches_[(size_t)b]->size()) throw std::runtime_error(pre + "a stale count out of range");
    stale_off[(size_t)b + 1] = stale_off[(size_t)b] + h[b];
  }
  retired = stale_off[(size_t)nb];
  const long candidates = h[nb], nonfinite = h[nb + 1];
  if (candidates < 0 || nonfinite < 0 || candidates + nonfinite > M) throw std::runtime_error(pre + "a detection count out of range");
  const long born = births ? lifecycle_born(candidates, p.max_births) : 0;
  if (retired > retired_cap)
    throw std::invalid_argument(pre + "retired_cap " + std::to_string(retired_cap) + " < " + std::to_string(retired) + " targets to retire");
  if (lifecycle_ids_wrap(p.first_id, born)) throw std::invalid_argument(pre + "the new ids wrap past 2^32 - 1");
  for (long j = 0; j < born; ++j)
    if (targets_.contains(p.first_id + (unsigned)j))
      throw std::invalid_argument(pre + "id " + std::to_string(p.first_id + (unsigned)j) + " of the new range exists already");
  int* lists = h + nb + 2;
  if (retired > 0) {
    off = 0;
    for (long b = 0; b < nb; ++b) {
      const long k = stale_off[(size_t)b + 1] - stale_off[(size_t)b];
      if (k > 0) TE_HIP_CHECK(hipMemcpyAsync(lists + stale_off[(size_t)b], s.list.get() + off, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, stream_));
      off += batches_[(size_t)b]->size();
    }
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  // the batch of the births, before anything is committed: a layout that is refused must leave everything as it was
  int birth_layout = 0;
  if (born > 0) birth_layout = chooseLayout(p.birth_type, p.Q, p.R, p.P0, 1);

  // THE COMMIT: counters, then retirements, then births
  off = 0;
  for (long b = 0; b < nb; ++b) {
    Batch& bt = *batches_[(size_t)b];
    const long n = bt.size();
    // (on the batch's own stream, ahead of its erase and append; the scratch was complete at the wait above)
    launch_lifecycle_commit(bt.track_miss_dev(), bt.track_hits_dev(), s.new_miss.get() + off, s.new_hits.get() + off, n, bt.stream());
    off += n;
  }
  std::vector<std::pair<unsigned, int>> moves;
  long at = 0;
  for (long b = 0; b < nb; ++b) {
    const long k = stale_off[(size_t)b + 1] - stale_off[(size_t)b];
    if (k <= 0) continue;
    Batch& bt = *batches_[(size_t)b];
    const int* slots = lists + stale_off[(size_t)b];
    for (long j = 0; j < k; ++j) {
      const unsigned id = bt.slot_id(slots[j]);
      retired_ids_out[at++] = id;
      targets_.erase(id);
    }
    bt.erase_slots(slots, k, moves);
    for (auto const& mv : moves) targets_.set(mv.first, Loc{(int)b, mv.second});
  }
  if (retired > 0) dev_ids_.dirty = true;
  if (born > 0) {
    int cls = 0;
    const int b = findOrCreateBatch(p.birth_type, p.Q, p.R, birth_layout, cls);
    std::vector<unsigned> ids((size_t)born);
    for (long j = 0; j < born; ++j) ids[(size_t)j] = p.first_id + (unsigned)j;
    const long first = batches_[(size_t)b]->append_gathered(born, ids.data(), p.t_birth, p.P0, cls, det_dev, s.list.get() + rows);
    targets_.reserve(targets_.size() + (size_t)born);
    for (long j = 0; j < born; ++j) targets_.set(ids[(size_t)j], Loc{b, (int)(first + j)});
    dev_ids_.dirty = true;
  }
  info[0] = retired; info[1] = born; info[2] = births ? candidates - born : 0; info[3] = births ? nonfinite : 0;
  info[4] = (long)p.first_id; info[5] = (long)p.first_id + born;
}

// ---------------------------------------------------------------- duplicate tracks (track_merge.hpp lists the launches)
void Shard::mergeSearch(double dt, double gate, long rounds, double cell, int min_hits, const MergeSlotOut* out, int* info_dev) {
  const int nb = (int)batches_.size();
  long rows = 0;
  for (auto& b : batches_) {
    const LayoutInfo L = b->layout();
    if (!assoc_table_launcher(b->type(), b->dtype(), L.g, L.layout, L.shared_axes != 0))
      throw std::logic_error("target_estimation_amd: find_duplicates: no kernel for this (model, precision, layout)");   // (never a fall-back)
    rows += b->size();
  }
  if (rows > 0x7fffffffL) throw std::invalid_argument("target_estimation_amd: find_duplicates: more than 2^31 - 1 targets on one device");
  const long buckets = plan_assoc_grid_buckets(rows, set_.assoc_grid_buckets);
  merge_.ensure(rows, buckets);
  std::vector<MergeBatchIn> in((size_t)nb);
  long off = 0;
  for (int b = 0; b < nb; ++b) {
    Batch& bt = *batches_[(size_t)b];
    bt.assoc_table_dev(dt, merge_.table.get() + off, b, nullptr, true);
    in[(size_t)b].size = bt.size(); in[(size_t)b].hits = bt.track_hits_dev(); in[(size_t)b].miss = bt.track_miss_dev();
    off += bt.size();
  }
  launch_merge_match(merge_, rows, in.data(), nb, gate, cell, (int)rounds, min_hits, buckets, stream_);
  off = 0;
  for (int b = 0; b < nb; ++b) {
    launch_merge_out(merge_, off, batches_[(size_t)b]->size(), out[b], stream_);
    off += batches_[(size_t)b]->size();
  }
  launch_merge_info(merge_, info_dev, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Shard::findDuplicatesDev(double dt, double gate, long rounds, double cell, int min_hits, const MergeSlotOut* out, long n_out, int* info_dev) {
  const std::string pre = "target_estimation_amd: find_duplicates: ";
  check_merge_args("find_duplicates", info_dev != nullptr, dt, gate, rounds, cell, min_hits, n_out, out != nullptr, 0, true);
  if (n_out != (long)batches_.size())
    throw std::invalid_argument(pre + "n_batches " + std::to_string(n_out) + " is not the manager's " + std::to_string(batches_.size()));
  for (size_t b = 0; b < batches_.size(); ++b)
    if (batches_[b]->size() > 0 && !out[b].dup) throw std::invalid_argument(pre + "dup_out_dev of a non-empty batch is NULL");
  mergeSearch(dt, gate, rounds, cell, min_hits, out, info_dev);
}

void Shard::retireDuplicates(double dt, double gate, long rounds, double cell, int min_hits, unsigned* retired_ids_out, unsigned* kept_ids_out,
                             long cap, long* info) {
  const std::string pre = "target_estimation_amd: retire_duplicates: ";
  check_merge_args("retire_duplicates", info != nullptr, dt, gate, rounds, cell, min_hits, 0, true, cap, retired_ids_out && kept_ids_out);
  const long nb = (long)batches_.size();
  long rows = 0;
  for (auto& b : batches_) rows += b->size();
  for (auto& b : batches_) b->prepare();   // the queued one-target steps and inits run first
  MergeScratch& s = merge_;
  s.ensure_retire(rows, nb);

  // THE PLAN, into the scratch alone
  std::vector<MergeSlotOut> outs((size_t)nb);
  long off = 0;
  for (long b = 0; b < nb; ++b) {
    outs[(size_t)b].dup = s.dup.get() + off; outs[(size_t)b].partner_batch = s.partner_batch.get() + off;
    outs[(size_t)b].partner_slot = s.partner_slot.get() + off;
    off += batches_[(size_t)b]->size();
  }
  int* info_dev = s.counts.get() + nb;
  mergeSearch(dt, gate, rounds, cell, min_hits, outs.data(), info_dev);
  off = 0;
  for (long b = 0; b < nb; ++b) {
    const long n = batches_[(size_t)b]->size();
    launch_lifecycle_compact(s.dup.get() + off, 1, n, s.csums.get(), s.list.get() + off, s.counts.get() + b, stream_);
    launch_merge_gather(s, off, n, s.counts.get() + b, stream_);
    off += n;
  }
  TE_HIP_CHECK(hipGetLastError());
  int* h = s.host.host();
  TE_HIP_CHECK(hipMemcpyAsync(h, s.counts.get(), sizeof(int) * (size_t)(nb + 4), hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  std::vector<long> dup_off((size_t)nb + 1, 0);   // where batch b's list lies behind the counts in the pinned block
  for (long b = 0; b < nb; ++b) {
    if (h[b] < 0 || h[b] > batches_[(size_t)b]->size()) throw std::runtime_error(pre + "a duplicate count out of range");
    dup_off[(size_t)b + 1] = dup_off[(size_t)b] + h[b];
  }
  const long retired = dup_off[(size_t)nb];
  const long rounds_run = h[nb + 1], settled = h[nb + 2], wide = h[nb + 3];
  if (retired > cap) throw std::invalid_argument(pre + "cap " + std::to_string(cap) + " < " + std::to_string(retired) + " targets to retire");
  int* lists = h + nb + 4;   // [retired] slots | [retired] partner batches | [retired] partner slots
  int* lists_b = lists + retired;
  int* lists_s = lists_b + retired;
  if (retired > 0) {
    off = 0;
    for (long b = 0; b < nb; ++b) {
      const long k = dup_off[(size_t)b + 1] - dup_off[(size_t)b];
      if (k > 0) {
        const size_t bytes = sizeof(int) * (size_t)k;
        TE_HIP_CHECK(hipMemcpyAsync(lists + dup_off[(size_t)b], s.list.get() + off, bytes, hipMemcpyDeviceToHost, stream_));
        TE_HIP_CHECK(hipMemcpyAsync(lists_b + dup_off[(size_t)b], s.list_batch.get() + off, bytes, hipMemcpyDeviceToHost, stream_));
        TE_HIP_CHECK(hipMemcpyAsync(lists_s + dup_off[(size_t)b], s.list_slot.get() + off, bytes, hipMemcpyDeviceToHost, stream_));
      }
      off += batches_[(size_t)b]->size();
    }
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  // both sides to ids BEFORE anything moves
  long at = 0;
  for (long b = 0; b < nb; ++b) {
    Batch& bt = *batches_[(size_t)b];
    for (long k = dup_off[(size_t)b]; k < dup_off[(size_t)b + 1]; ++k, ++at) {
      const int slot = lists[k], pb = lists_b[k], ps = lists_s[k];
      if (slot < 0 || slot >= bt.size() || pb < 0 || pb >= nb || ps < 0 || ps >= batches_[(size_t)pb]->size())
        throw std::runtime_error(pre + "a duplicate or its partner out of range");
      retired_ids_out[at] = bt.slot_id(slot);
      kept_ids_out[at] = batches_[(size_t)pb]->slot_id(ps);
    }
  }
  // THE COMMIT
  std::vector<std::pair<unsigned, int>> moves;
  at = 0;
  for (long b = 0; b < nb; ++b) {
    const long k = dup_off[(size_t)b + 1] - dup_off[(size_t)b];
    if (k <= 0) continue;
    Batch& bt = *batches_[(size_t)b];
    for (long j = 0; j < k; ++j) targets_.erase(retired_ids_out[at++]);
    bt.erase_slots(lists + dup_off[(size_t)b], k, moves);
    for (auto const& mv : moves) targets_.set(mv.first, Loc{(int)b, mv.second});
  }
  if (retired > 0) dev_ids_.dirty = true;
  info[0] = retired; info[1] = rounds_run; info[2] = settled; info[3] = wide;
}

void Shard::launchRows(double* pose_out) {
  for (size_t b = 0; b < batches_.size(); ++b)
    if (batches_[b]->size() > 0) batches_[b]->outputs_rows_dev(pose_out, rank_maps_[b].dev.get());
}

}  // namespace te
