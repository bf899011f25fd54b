// batch_store.cpp -- see batch_store.hpp.
#include "batch_store.hpp"
#include "measured_pose.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "hip_check.hpp"
#include "intersect_gate.hpp"

namespace te {

namespace {
std::mutex g_live_mu;
std::vector<void*> g_deferred_frees;
int g_live_sessions = 0;
double g_live_share = 0.0;
}  // namespace

void device_free(void* p) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lg(g_live_mu);
    if (g_live_sessions > 0) { g_deferred_frees.push_back(p); return; }
  }
  (void)hipFree(p);
}

bool live_session_begin(double share) {
  std::lock_guard<std::mutex> lg(g_live_mu);
  const char* e = std::getenv("TE_LIVE_IGNORE_OTHERS");   // tests: the start-word path of a grid that does not become resident
  if (!(e && e[0] == '1') && g_live_sessions > 0 && g_live_share + share > 1.0) return false;
  ++g_live_sessions;
  g_live_share += share;
  return true;
}

void live_session_ended(double share) {
  std::vector<void*> drain;
  {
    std::lock_guard<std::mutex> lg(g_live_mu);
    g_live_share -= share;
    if (--g_live_sessions > 0) return;
    g_live_sessions = 0; g_live_share = 0.0;
    drain.swap(g_deferred_frees);
  }
  for (void* p : drain) (void)hipFree(p);
}

double live_sessions_share() {
  std::lock_guard<std::mutex> lg(g_live_mu);
  return g_live_share;
}


const Ops* get_ops(int type, int dtype, int g) {
  if (g == kLanesSeparableShared) {   // the shared-axes storage form of 301: fp64 only
    if (dtype != F64) return nullptr;
    switch (type) {
      case UNIFORM_VELOCITY: return get_ops_shared_uv();
      case UNIFORM_ACCELERATION: return get_ops_shared_ua();
      case ANGULAR_RATES: return get_ops_shared_ar();
      case ANGULAR_VELOCITIES: return get_ops_shared_av();
      default: return nullptr;
    }
  }
  switch (type) {
    case UNIFORM_VELOCITY: return get_ops_uv(dtype, g);
    case UNIFORM_ACCELERATION: return get_ops_ua(dtype, g);
    case ANGULAR_RATES: return get_ops_ar(dtype, g);
    case ANGULAR_VELOCITIES: return get_ops_av(dtype, g);
    default: return nullptr;
  }
}

Batch::Batch(int type, int dtype, int lanes, const double* Q, const double* R, hipStream_t stream, std::mutex* owner_lock, bool allow_shared,
             bool allow_uniform_tiles)
    : type_(type), dtype_(dtype), lanes_code_(lanes), owner_lock_(owner_lock), ops_(get_ops(type, dtype, lanes)), stream_(stream), ut_on_(allow_uniform_tiles) {
  if (!ops_) throw std::runtime_error("target_estimation_amd: unsupported (model, precision, lanes-per-target) combination");
  if (allow_shared && lanes == kLanesSeparablePacked && dtype == F64 && shared_axes_qr_ok(type, Q, R)) {
    const Ops* shared = get_ops(type, dtype, kLanesSeparableShared);
    if (shared) ops_ = shared;
  }
  add_class(Q, R);
}

void Batch::demote_shared() {
  if (!shared_axes()) return;
  flush();   // queued creations and one-target steps are for the records as they are
  const Ops* plain = get_ops(type_, dtype_, lanes_code_);
  if (cap_ > 0) {
    const size_t bytes = (size_t)(cap_ / plain->L.tpw) * (size_t)plain->L.tile_bytes;
    DeviceBuf<char> rec;
    rec.alloc(bytes);
    TE_HIP_CHECK(hipMemsetAsync(rec.get(), 0, bytes, stream_));
    ops_->expand(records(), rec.get(), n_, stream_);
    TE_HIP_CHECK(hipGetLastError());
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    d_rec_ = std::move(rec);
    d_tile_blk_.reset(); d_tile_uni_.reset();   // (the plain form has no uniform tiles)
    d_rec_alt_.reset(); alt_failed_ = false;   // re-created in the plain form by the next A -> B tick
  }
  ops_ = plain;
  cache_valid_ = false;
  drop_graphs();   // (the manager's all-batches recordings miss on dev_identity().ops)
}

static std::string class_key(const double* Q, int nq, const double* R, int nr) {
  std::string k((size_t)(nq + nr) * sizeof(double), '\0');
  std::memcpy(&k[0], Q, (size_t)nq * sizeof(double));
  std::memcpy(&k[(size_t)nq * sizeof(double)], R, (size_t)nr * sizeof(double));
  return k;
}

int Batch::find_class(const double* Q, const double* R) const {
  const int n = ops_->L.n, m = ops_->L.m;
  auto it = class_index_.find(class_key(Q, n * n, R, m * m));
  return it == class_index_.end() ? -1 : it->second;
}

int Batch::add_class(const double* Q, const double* R) {
  if (n_classes_ >= 1) demote_shared();   // the shared-axes form has no per-class kernels
  const int n = ops_->L.n, m = ops_->L.m;
  const bool sep = ops_->L.layout == LAYOUT_SEPARABLE || ops_->L.layout == LAYOUT_SEPARABLE_PACKED;
  const int words = qr_words(type_, sep);   // te_layout.hpp: full [Q | R], or only the in-group entries (separable layouts)
  const size_t es = elem_size();
  if (n_classes_ == qr_cap_) {   // grow the device table (geometric); recorded graphs hold the old pointer
    const int want = qr_cap_ ? qr_cap_ * 2 : 1;
    DeviceBuf<char> nt;
    nt.alloc((size_t)want * words * es);
    if (n_classes_ > 0) {
      TE_HIP_CHECK(hipStreamSynchronize(stream_));
      TE_HIP_CHECK(hipMemcpy(nt.get(), d_qr_.get(), (size_t)n_classes_ * words * es, hipMemcpyDeviceToDevice));
    }
    d_qr_ = std::move(nt);
    qr_cap_ = want;
    drop_graphs();
  }
  std::vector<unsigned char> host((size_t)words * es);
  auto put = [&](int w, double v) {
    if (w < 0) return;   // an entry between different axis groups: zero by the separable layout's precondition
    if (dtype_ == F64) reinterpret_cast<double*>(host.data())[w] = v;
    else reinterpret_cast<float*>(host.data())[w] = (float)v;
  };
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) put(qr_q_word(type_, sep, r, c), Q[r * n + c]);
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) put(qr_r_word(type_, sep, r, c), R[r * m + c]);
  TE_HIP_CHECK(hipMemcpy(d_qr_.get() + (size_t)n_classes_ * words * es, host.data(), host.size(), hipMemcpyHostToDevice));
  class_index_.emplace(class_key(Q, n * n, R, m * m), n_classes_);
  class_qr_.emplace_back((size_t)(n * n + m * m));
  std::copy(Q, Q + n * n, class_qr_.back().begin());
  std::copy(R, R + m * m, class_qr_.back().begin() + n * n);
  if (n_classes_ == 1) drop_graphs();   // the single-class kernels were recorded: from now on the per-class ones run
  return n_classes_++;
}

namespace {
// batched erase: the rejection runs of the survivors that fill the holes (sources lie above every destination)
__global__ void run_moves_kernel(unsigned char* run, const int* src, const int* dst, long m) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) run[dst[i]] = run[src[i]];
}
}  // namespace

void Batch::run_move(long src, long dst) {
  if (d_run_) TE_HIP_CHECK(hipMemcpyAsync(d_run_.get() + dst, d_run_.get() + src, 1, hipMemcpyDeviceToDevice, stream_));
  if (d_miss_) {   // the track counters follow their target as the run does
    TE_HIP_CHECK(hipMemcpyAsync(d_miss_.get() + dst, d_miss_.get() + src, 1, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(d_hits_.get() + dst, d_hits_.get() + src, 1, hipMemcpyDeviceToDevice, stream_));
  }
  p0idx_dirty_.mark(dst, 1);
}

void Batch::prepare_reacquire(const InnovStream& innov) {
  if (!innov.reacq.on || n_ == 0) return;
  prepare_p0_tables();
}

void Batch::prepare_p0_tables() {
  const size_t nn = (size_t)ops_->L.n * (size_t)ops_->L.n;
  if (!p0_kept_ || slot_p0_.size() < (size_t)n_) throw std::runtime_error("target_estimation_amd: re-acquisition: the batch does not keep its initial covariances");
  const P0TableMirror::Upload u = p0tab_dev_.plan((long)p0_tab_.size());
  if (u.grow) {   // recorded sequences hold the old table
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    drop_graphs();
    const P0TableMirror planned = p0tab_dev_;
    p0tab_dev_.reset();   // (an allocation that throws leaves an empty table, which the next call builds whole)
    d_p0tab_.alloc(nn * (size_t)u.new_cap);
    p0tab_dev_ = planned;
  }
  if (u.count > 0) {
    std::vector<double> rows(nn * (size_t)u.count);
    for (long r = 0; r < u.count; ++r) std::copy(p0_tab_[(size_t)(u.first + r)].begin(), p0_tab_[(size_t)(u.first + r)].end(), rows.begin() + (size_t)r * nn);
    TE_HIP_CHECK(hipMemcpyAsync(d_p0tab_.get() + (size_t)u.first * nn, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, stream_));
    TE_HIP_CHECK(hipStreamSynchronize(stream_));   // (rows goes out of scope)
  }
  p0idx_dirty_.clip(n_);
  if (!p0idx_dirty_.empty()) {
    TE_HIP_CHECK(hipMemcpyAsync(d_p0idx_.get() + p0idx_dirty_.lo, slot_p0_.data() + p0idx_dirty_.lo, sizeof(int) * (size_t)(p0idx_dirty_.hi - p0idx_dirty_.lo),
                                hipMemcpyHostToDevice, stream_));
    TE_HIP_CHECK(hipStreamSynchronize(stream_));   // (slot_p0_ may change before the copy has run)
    p0idx_dirty_.clear();
  }
}

void Batch::fill_reacquire(StepParams& p, const InnovStream& innov, long s_call) const {
  if (!innov.reacq.on) return;
  p.reacq = 1; p.reacq_k = innov.reacq.k; p.reacq_run = d_run_.get(); p.reacq_event = innov.reacq.row(s_call);
  p.reacq_p0 = d_p0tab_.get(); p.reacq_p0_idx = d_p0idx_.get();
}

void Batch::set_update_gate(const UpdateGate& g) {
  check_update_gate(g.nis_max, g.max_rejects);
  touch();   // what is queued was queued under the policy it runs under
  pol_ = g;
}

const char* Batch::update_gate_refusal(const UpdateGate& g) const {
  if (!g.on()) return nullptr;
  if (ops_->L.layout != LAYOUT_SEPARABLE && ops_->L.layout != LAYOUT_SEPARABLE_PACKED)
    return "target_estimation_amd: update gate: not served by id for a batch of the dense layouts (coupled matrices): no gated indexed kernel";
  if (n_classes_ > 1) return "target_estimation_amd: update gate: not served by id for a batch with several (Q, R) classes: no gated indexed kernel";
  if (keep_meas_) return "target_estimation_amd: update gate: not served by id for a batch that keeps measured poses (set_keep_measurement)";
  if (g.max_rejects >= 0 && !p0_kept_) return "target_estimation_amd: update gate: max_rejects >= 0: the batch no longer keeps its initial covariances";
  return nullptr;
}

void Batch::pol_reserve(long k) {
  if (k <= pol_cap_) return;
  const long want = (std::max<long>(std::max<long>(k, 64), pol_cap_ * 2) + 15) / 16 * 16;
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  pol_cap_ = 0; d_pol_ = nullptr;
  h_pol_.alloc((size_t)want * (sizeof(double) + 1) + 64, kPinnedMapped);
  d_pol_ = h_pol_.dev();
  pol_cap_ = want;
}

void Batch::fill_update_gate(StepParams& p, long k, double* nis_dev, unsigned char* event_dev) {
  if (const char* why = update_gate_refusal()) throw std::runtime_error(why);
  if (!nis_dev) { pol_reserve(k); nis_dev = pol_nis_dev(); event_dev = pol_event_dev(); }
  p.gate = pol_.nis_max; p.gate_id = 1; p.gate_id_k = pol_.max_rejects;
  p.nis = nis_dev; p.gate_id_event = event_dev;
  if (pol_.max_rejects >= 0) {
    prepare_p0_tables();
    p.reacq_run = d_run_.get(); p.reacq_p0 = d_p0tab_.get(); p.reacq_p0_idx = d_p0idx_.get();
  }
}

void Batch::rejection_runs(unsigned char* out) {
  flush();
  if (n_ <= 0) return;
  TE_HIP_CHECK(hipMemcpyAsync(out, d_run_.get(), (size_t)n_, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::track_counts(unsigned char* miss_out, unsigned char* hits_out) {
  flush();
  if (n_ <= 0) return;
  if (miss_out) TE_HIP_CHECK(hipMemcpyAsync(miss_out, d_miss_.get(), (size_t)n_, hipMemcpyDeviceToHost, stream_));
  if (hits_out) TE_HIP_CHECK(hipMemcpyAsync(hits_out, d_hits_.get(), (size_t)n_, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::track_count(long slot, int& miss, int& hits) {
  flush();
  if (slot < 0 || slot >= n_) throw std::runtime_error("target_estimation_amd: track_count: bad slot");
  unsigned char c[2] = {0, 0};
  TE_HIP_CHECK(hipMemcpyAsync(&c[0], d_miss_.get() + slot, 1, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipMemcpyAsync(&c[1], d_hits_.get() + slot, 1, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  miss = (int)c[0]; hits = (int)c[1];
}

int Batch::rejection_run(long slot) {
  flush();
  if (slot < 0 || slot >= n_) throw std::runtime_error("target_estimation_amd: rejection_run: bad slot");
  unsigned char c = 0;
  TE_HIP_CHECK(hipMemcpyAsync(&c, d_run_.get() + slot, 1, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  return (int)c;
}

void Batch::launch_step(const StepParams& p, hipStream_t st, int meas_rows) {
  const bool gated_rows = keep_meas_ && p.gate > 0.0;
  if (gated_rows) {   // the measured-pose rows keep ACCEPTED measurements: the gate's mask comes from the writer, for the row kernel too
    StepParams q = p;
    q.gate_by_writer = 1;
    ops_->step(q, st);
  } else {
    ops_->step(p, st);
  }
  if (!keep_meas_ || !p.meas || p.n <= 0) return;
  const unsigned char* has = gated_rows ? p.gate_row : p.has_meas;
  const long has_stride = gated_rows ? 0 : p.has_stride;
  const unsigned blocks = (unsigned)((p.n + 255) / 256);
  if (dtype_ == F64)
    keep_measurement_kernel<double><<<blocks, 256, 0, st>>>(static_cast<const double*>(p.meas), p.meas_ld, p.tick_stride, has, has_stride,
                                                            p.n_ticks, p.idx, p.n, meas_rows, d_lastmeas_.get());
  else
    keep_measurement_kernel<float><<<blocks, 256, 0, st>>>(static_cast<const float*>(p.meas), p.meas_ld, p.tick_stride, has, has_stride,
                                                           p.n_ticks, p.idx, p.n, meas_rows, d_lastmeas_.get());
}

void Batch::set_keep_measurement(bool on) {
  if (on == keep_meas_) return;
  touch();
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  drop_graphs();   // recorded sequences do (not) contain the row kernels
  if (on) {
    if (cap_ > 0) {
      d_lastmeas_.alloc(7 * (size_t)cap_);
      init_measured_rows_kernel<<<(unsigned)((cap_ * 7 + 255) / 256), 256, 0, stream_>>>(d_lastmeas_.get(), 0, cap_);
      TE_HIP_CHECK(hipGetLastError());
    }
  } else {
    d_lastmeas_.reset();
  }
  keep_meas_ = on;
}

void Batch::measured_poses(const int* slots, long n, double* out) {
  if (!keep_meas_) throw std::runtime_error("target_estimation_amd: measured poses are not kept (target_manager_set_keep_measurement)");
  flush();
  if (n <= 0) return;
  if (!slots) {
    TE_HIP_CHECK(hipMemcpyAsync(out, d_lastmeas_.get(), sizeof(double) * 7 * (size_t)n, hipMemcpyDeviceToHost, stream_));
  } else {
    for (long i = 0; i < n; ++i)
      TE_HIP_CHECK(hipMemcpyAsync(out + 7 * i, d_lastmeas_.get() + 7 * (long)slots[i], sizeof(double) * 7, hipMemcpyDeviceToHost, stream_));
  }
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::class_matrices(long slot, double* Q, double* R) {
  const int n = ops_->L.n, m = ops_->L.m;
  int cls = 0;
  if (n_classes_ > 1) {
    flush();
    TE_HIP_CHECK(hipMemcpyAsync(&cls, d_cls_.get() + slot, sizeof(int), hipMemcpyDeviceToHost, stream_));
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  const std::vector<double>& qr = class_qr_.at((size_t)cls);
  if (Q) std::copy(qr.begin(), qr.begin() + n * n, Q);
  if (R) std::copy(qr.begin() + n * n, qr.begin() + n * n + m * m, R);
}

int Batch::intern_p0(const double* P0) {
  if (!p0_kept_) return -1;
  const int n = ops_->L.n;
  std::string key(reinterpret_cast<const char*>(P0), sizeof(double) * (size_t)n * n);
  auto it = p0_index_.find(key);
  if (it != p0_index_.end()) return it->second;
  if (p0_tab_.size() >= kP0TableMax) {   // too many distinct initial covariances to mirror on the host: stop keeping them
    p0_kept_ = false;
    p0_tab_.clear(); p0_index_.clear(); slot_p0_.clear();
    return -1;
  }
  p0_tab_.emplace_back(P0, P0 + (size_t)n * n);
  p0_index_.emplace(std::move(key), (int)p0_tab_.size() - 1);
  return (int)p0_tab_.size() - 1;
}

bool Batch::initial_covariance(long slot, double* P0) {
  if (!p0_kept_ || slot < 0 || (size_t)slot >= slot_p0_.size()) return false;
  const std::vector<double>& v = p0_tab_[(size_t)slot_p0_[(size_t)slot]];
  std::copy(v.begin(), v.end(), P0);
  return true;
}

long Batch::promote_after() {
  static const long v = [] { const char* e = std::getenv("TE_UNIFORM_TILES_AFTER"); const long k = e ? std::atol(e) : 2L; return k < 0 ? 0L : k; }();
  return v;
}

void Batch::settle_tiles() {
  dense_streak_ = 0;
  if (!ut_flagged_) return;
  ut_flagged_ = false;
  if (!d_tile_uni_) return;
  if (n_ > 0 && ops_->settle) {
    ops_->settle(d_rec_.get(), n_, d_tile_blk_.get(), d_tile_uni_.get(), stream_);
    TE_HIP_CHECK(hipGetLastError());
  }
  // (also for a batch emptied by erases: its flags would otherwise outlive the targets they described)
  TE_HIP_CHECK(hipMemsetAsync(d_tile_uni_.get(), 0, sizeof(int) * (size_t)(cap_ / ops_->L.tpw), stream_));
}

long Batch::count_uniform(long* targets_in_them) {
  if (targets_in_them) *targets_in_them = 0;
  if (!ut_flagged_ || !d_tile_uni_ || n_ <= 0) return 0;
  const long tpw = ops_->L.tpw, tiles = (n_ + tpw - 1) / tpw;
  std::vector<int> h((size_t)tiles);
  TE_HIP_CHECK(hipMemcpyAsync(h.data(), d_tile_uni_.get(), sizeof(int) * (size_t)tiles, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  long k = 0, targets = 0;
  for (long t = 0; t < tiles; ++t)
    if (h[(size_t)t] != 0) { ++k; targets += std::min(tpw, n_ - t * tpw); }
  if (targets_in_them) *targets_in_them = targets;
  return k;
}

long Batch::uniform_tiles() {
  flush();   // (a queued one-target step settles the tiles when it runs: it has happened as far as the caller knows)
  return count_uniform(nullptr);
}

StepParams Batch::dense_params() {
  StepParams p;
  p.rec = d_rec_.get(); p.qr = d_qr_.get(); p.cls = n_classes_ > 1 ? d_cls_.get() : nullptr; p.n = n_; p.idx = nullptr;
  p.meas = nullptr; p.meas_ld = 0; p.has_meas = nullptr; p.dt_per = nullptr; p.dt = 0.0;
  p.t_base = d_tbase_.get(); p.nm_base = d_nmbase_.get();
  p.gate_row = d_has_eff_.get();
  if (uniform_tiles_enabled() && d_tile_uni_) {
    p.tile_blk = d_tile_blk_.get(); p.tile_uni = d_tile_uni_.get();
    p.promote = (recording_ || dense_streak_ >= promote_after()) ? 1 : 0;
    if (!recording_) {   // (a recording launches nothing: note_replay() when it is replayed)
      if (p.promote) ut_flagged_ = true;
      ++dense_streak_;
    }
  }
  return p;
}

StepParams Batch::base_params() {
  StepParams p;
  p.rec = records(); p.qr = d_qr_.get(); p.cls = n_classes_ > 1 ? d_cls_.get() : nullptr; p.n = n_; p.idx = nullptr;
  p.meas = nullptr; p.meas_ld = 0; p.has_meas = nullptr; p.dt_per = nullptr; p.dt = 0.0;
  p.t_base = d_tbase_.get(); p.nm_base = d_nmbase_.get();
  return p;
}

Batch::~Batch() {
  if (live_.active) { try { live_stop(); } catch (...) {} }
  if (live_.zombie && live_.stream) (void)hipStreamSynchronize(live_.stream.get());   // (told to stop: it ends as soon as it starts)
  live_release();
  (void)hipStreamSynchronize(stream_);
  drop_graphs();
}   // (everything else is the members': batch_store.hpp on their order)

long Batch::zigzag_min_bytes() {
  static const long v = [] { const char* e = std::getenv("TE_ZIGZAG_MIN_MB"); return (e ? std::atol(e) : 128L) << 20; }();
  return v;
}

long Batch::pingpong_min_bytes() {
  static const long v = [] { const char* e = std::getenv("TE_PINGPONG_MIN_MB"); const long mb = e ? std::atol(e) : 1536L; return mb < 0 ? -1L : mb << 20; }();
  return v;
}

char* Batch::alt_records() {
  if (!d_rec_alt_ && !alt_failed_) {   // same capacity as d_rec_; zero-filled so that the idle lanes of a ragged last tile hold defined words
    const size_t bytes = (size_t)(cap_ / ops_->L.tpw) * (size_t)ops_->L.tile_bytes;
    if (!d_rec_alt_.try_alloc(bytes)) {   // no room for a second copy of the state: stay in place (same results)
      alt_failed_ = true;
      return nullptr;
    }
    TE_HIP_CHECK(hipMemsetAsync(d_rec_alt_.get(), 0, bytes, stream_));
  }
  return d_rec_alt_.get();
}

void Batch::synchronize() {
  flush();
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

long Batch::algorithmic_bytes_per_cycle() {
  const long n = ops_->L.n;
  const bool angular = (type_ == ANGULAR_RATES || type_ == ANGULAR_VELOCITIES);
  // full P: 2n + 2n^2 + 7 (+6); symmetric-packed P: 2n + n(n+1) + 7 (+6)
  long pwords = 2 * n * n;
  if (ops_->L.layout == LAYOUT_PACKED) pwords = n * (n + 1);
  if (ops_->L.layout == LAYOUT_SEPARABLE || ops_->L.layout == LAYOUT_SEPARABLE_PACKED) {
    // only the entries inside an axis group exist (the others are structural zeros): read + write; in the shared-axes form
    // only those of the first axis of every kind (te_layout.hpp share_rep): the form's own, smaller figure
    pwords = 0;
    for (int r = 0; r < n; ++r)
      for (int c = (ops_->L.layout == LAYOUT_SEPARABLE_PACKED ? r : 0); c < n; ++c)
        pwords += (group_of(type_, r) == group_of(type_, c) && (!shared_axes() || share_rep(type_, r) == r)) ? 2 : 0;
  }
  // measurement words the step kernel READS: [x y z] for the linear models, [x y z qx qy qz qw] for the angular
  // ones (kf_step_sep.hpp MW, kf_step.hpp ymeas_own/qmeas); SURVEY 8d's formula charges 7 for every model
  const long full = (2 * n + pwords + (angular ? 7 + 6 : 3)) * (long)elem_size();
  // Uniform tiles: what the NEXT dense tick moves, given the flags as they are.  A flagged tile's targets move 16 B less per
  // linear-covariance chunk, read and written, and the tile moves its block (LW words read and written) and its flag (4 B);
  // every other tile as ever.  The mean over the batch, rounded down (the roofline fraction is never flattered); with no tile
  // flagged, exactly the figure above.
  if (!uniform_tiles_enabled()) return full;
  flush();   // (as uniform_tiles(): a queued one-target step settles the tiles when it runs)
  long in_them = 0;
  const long k = count_uniform(&in_them);
  if (k == 0) return full;
  const long total = n_ * full - in_them * 2L * 16L * ops_->L.lin_chunks + k * (2L * 8L * ops_->L.lin_words + 4L);
  return total / n_;
}


void Batch::reserve(long n) {
  if (n <= cap_) return;
  settle_tiles();   // (the records move as plain records; the new tile arrays start with no tile flagged)
  const long tpw = ops_->L.tpw;
  long want = std::max(n, cap_ * 2);
  want = (want + tpw - 1) / tpw * tpw;
  const size_t new_bytes = (size_t)(want / tpw) * (size_t)ops_->L.tile_bytes;
  const size_t tiles = uniform_tiles_enabled() ? (size_t)(want / tpw) : 0;   // about 1.5 B per target (angular_rates: 96 + 4 B per 64)
  // Every new array first, into local owners: a throw anywhere before the commit below leaves the batch exactly as it was.
  DeviceBuf<char> rec;
  DeviceBuf<TClock> tb;
  DeviceBuf<int> nm, cl, p0idx, uni;
  DeviceBuf<double> lm, blk;
  DeviceBuf<unsigned char> has_eff, run, miss, hits;
  rec.alloc(new_bytes);
  tb.alloc((size_t)want);
  nm.alloc((size_t)want);
  cl.alloc((size_t)want);
  if (keep_meas_) lm.alloc(7 * (size_t)want);
  has_eff.alloc((size_t)want);   // (the gate's mask row is written whole by every launch that reads it: no contents to carry over)
  run.alloc((size_t)want);
  miss.alloc((size_t)want);
  hits.alloc((size_t)want);
  p0idx.alloc((size_t)want);
  if (tiles) { blk.alloc(tiles * (size_t)ops_->L.lin_words); uni.alloc(tiles); }
  TE_HIP_CHECK(hipMemsetAsync(rec.get(), 0, new_bytes, stream_));
  TE_HIP_CHECK(hipMemsetAsync(tb.get(), 0, sizeof(TClock) * want, stream_));
  TE_HIP_CHECK(hipMemsetAsync(nm.get(), 0, sizeof(int) * want, stream_));
  TE_HIP_CHECK(hipMemsetAsync(cl.get(), 0, sizeof(int) * want, stream_));
  if (cap_ > 0) {
    TE_HIP_CHECK(hipMemcpyAsync(rec.get(), d_rec_.get(), (size_t)(cap_ / tpw) * (size_t)ops_->L.tile_bytes, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(tb.get(), d_tbase_.get(), sizeof(TClock) * cap_, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(nm.get(), d_nmbase_.get(), sizeof(int) * cap_, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(cl.get(), d_cls_.get(), sizeof(int) * cap_, hipMemcpyDeviceToDevice, stream_));
  }
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  if (lm && d_lastmeas_ && cap_ > 0) TE_HIP_CHECK(hipMemcpy(lm.get(), d_lastmeas_.get(), sizeof(double) * 7 * (size_t)cap_, hipMemcpyDeviceToDevice));
  // the rejection runs follow their targets; the slot -> row index is uploaded again from the host's (prepare_reacquire)
  TE_HIP_CHECK(hipMemsetAsync(run.get(), 0, (size_t)want, stream_));
  if (d_run_ && n_ > 0) TE_HIP_CHECK(hipMemcpyAsync(run.get(), d_run_.get(), (size_t)n_, hipMemcpyDeviceToDevice, stream_));
  // ... and so do the track counters
  TE_HIP_CHECK(hipMemsetAsync(miss.get(), 0, (size_t)want, stream_));
  TE_HIP_CHECK(hipMemsetAsync(hits.get(), 0, (size_t)want, stream_));
  if (d_miss_ && n_ > 0) {
    TE_HIP_CHECK(hipMemcpyAsync(miss.get(), d_miss_.get(), (size_t)n_, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(hits.get(), d_hits_.get(), (size_t)n_, hipMemcpyDeviceToDevice, stream_));
  }
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  if (tiles) {
    TE_HIP_CHECK(hipMemsetAsync(blk.get(), 0, sizeof(double) * tiles * (size_t)ops_->L.lin_words, stream_));
    TE_HIP_CHECK(hipMemsetAsync(uni.get(), 0, sizeof(int) * tiles, stream_));
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  // The commit: nothing below throws.  The old arrays are released here, behind every synchronisation above, in the old order
  // (the price of all-or-nothing: until here the old records coexist with ALL the new arrays, not only with the new records).
  d_rec_ = std::move(rec); d_tbase_ = std::move(tb); d_nmbase_ = std::move(nm); d_cls_ = std::move(cl);
  d_rec_alt_.reset(); alt_failed_ = false;   // re-created at the new capacity by the next A -> B tick
  if (keep_meas_) d_lastmeas_ = std::move(lm);
  d_has_eff_ = std::move(has_eff);
  d_run_ = std::move(run);
  d_miss_ = std::move(miss); d_hits_ = std::move(hits);
  d_p0idx_ = std::move(p0idx);
  p0idx_dirty_.clear(); p0idx_dirty_.mark(0, want);
  d_tile_blk_ = std::move(blk); d_tile_uni_ = std::move(uni);
  cap_ = want;
  drop_graphs();
}

void Batch::stage_reserve(long n) {
  if (n <= stage_cap_) return;
  const long want = std::max(n, stage_cap_ * 2);
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  // (nothing to carry over, and up to hundreds of MB: released before the new blocks exist; a throw leaves an empty staging area)
  stage_cap_ = 0;
  d_idx_.reset(); d_aos_.reset(); d_meas_.reset(); d_mask_.reset(); d_dtper_.reset();
  d_dtper_.alloc((size_t)want);
  d_idx_.alloc((size_t)want);
  d_aos_.alloc(19 * (size_t)want);
  d_meas_.alloc(elem_size() * 7 * (size_t)want);
  d_mask_.alloc((size_t)want);
  stage_cap_ = want;
}

void Batch::upload_slots(const int* slots, long n) {
  TE_HIP_CHECK(hipMemcpyAsync(d_idx_.get(), slots, sizeof(int) * n, hipMemcpyHostToDevice, stream_));
}

long Batch::append(long count, const unsigned* ids, double t0, const double* P0, bool per_target_P0,
                   const double* p0, const double* v0, const double* a0, int cls, const int* cls_of, const int* P0_index,
                   long P0_count) {
  const int N = ops_->L.n;
  // the shared-axes form rests on every initial covariance having equal blocks on the axes of a kind: one that has not ends it
  if (count > 0 && shared_axes() && !shared_axes_p0_ok(type_, P0, P0_index ? P0_count : (per_target_P0 ? count : 1))) demote_shared();
  // ONE target (the reference's TargetManager::init, called target by target): queued.  The slot, its id and the host
  // mirrors exist at once; the record is written by the next flush() -- one init launch for a whole run of creations with
  // the same (t0, P0, class) instead of three copies, a launch and a synchronisation each (28 us -> 0.3 us per target).
  if (count == 1 && !per_target_P0 && !cls_of && !P0_index && v0 && a0 && n_ < cap_ && !live_.active) {
    InitQueue& q = initq_;
    if (!q.ids.empty() && (t0 != q.t0 || cls != q.cls || std::memcmp(P0, q.P0.data(), sizeof(double) * (size_t)N * N) != 0)) flush_inits();
    if (q.ids.empty()) { q.t0 = t0; q.cls = cls; q.P0.assign(P0, P0 + (size_t)N * N); q.first = n_; }
    q.ids.push_back(ids[0]);
    q.p0.insert(q.p0.end(), p0, p0 + 7);
    q.v0.insert(q.v0.end(), v0, v0 + 6);
    q.a0.insert(q.a0.end(), a0, a0 + 6);
    cache_valid_ = false;   // the getter table is laid out by n_
    nm_valid_ = false; nm_reads_ = 0;
    if (p0_kept_) {
      slot_p0_.resize((size_t)n_, 0);
      const int r = intern_p0(P0);
      if (p0_kept_) slot_p0_.push_back(r);
    }
    slot_ids_.push_back(ids[0]);
    return n_++;
  }
  touch();
  if (count <= 0) return n_;
  return append_now(n_, count, ids, t0, P0, per_target_P0, p0, v0, a0, cls, cls_of, P0_index, P0_count, true);
}

void Batch::flush_inits() {
  InitQueue& q = initq_;
  if (q.ids.empty()) return;
  InitQueue w;
  w.ids.swap(q.ids); w.p0.swap(q.p0); w.v0.swap(q.v0); w.a0.swap(q.a0); w.P0.swap(q.P0);   // (append_now synchronises: nothing re-enters)
  append_now(q.first, (long)w.ids.size(), w.ids.data(), q.t0, w.P0.data(), false, w.p0.data(), w.v0.data(), w.a0.data(), q.cls, nullptr, nullptr, 0, false);
}

// The device side of append (and, with `bookkeeping`, the host side of a multi-target append): records first .. first + count.
long Batch::append_now(long first, long count, const unsigned* ids, double t0, const double* P0, bool per_target_P0,
                       const double* p0, const double* v0, const double* a0, int cls, const int* cls_of, const int* P0_index,
                       long P0_count, bool bookkeeping, const double* gather_det_dev, const int* gather_rows_dev) {
  const int N = ops_->L.n;
  reserve(first + count);
  stage_reserve((cls_of || P0_index) ? 3 * count : count);   // slot list (+ per-entry class and P0 indices)
  std::vector<int> slots((size_t)count);
  for (long i = 0; i < count; ++i) slots[(size_t)i] = (int)(first + i);
  upload_slots(slots.data(), count);
  double* d_p0 = d_aos_.get();
  double* d_v0 = d_aos_.get() + 7 * count;
  double* d_a0 = d_aos_.get() + 13 * count;
  if (gather_det_dev) launch_lifecycle_gather(gather_det_dev, gather_rows_dev, count, d_p0, stream_);   // (the rows never leave the device)
  else TE_HIP_CHECK(hipMemcpyAsync(d_p0, p0, sizeof(double) * 7 * count, hipMemcpyHostToDevice, stream_));
  if (v0) TE_HIP_CHECK(hipMemcpyAsync(d_v0, v0, sizeof(double) * 6 * count, hipMemcpyHostToDevice, stream_));
  if (a0) TE_HIP_CHECK(hipMemcpyAsync(d_a0, a0, sizeof(double) * 6 * count, hipMemcpyHostToDevice, stream_));
  const long p0_words = (P0_index ? P0_count : (per_target_P0 ? count : 1)) * (long)N * N;
  if (p0_words > P0_cap_) {
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    P0_cap_ = 0;
    d_P0_.alloc((size_t)p0_words);
    P0_cap_ = p0_words;
  }
  TE_HIP_CHECK(hipMemcpyAsync(d_P0_.get(), P0, sizeof(double) * p0_words, hipMemcpyHostToDevice, stream_));
  InitArgs a;
  a.rec = records(); a.idx = d_idx_.get(); a.n = count; a.p0 = d_p0; a.v0 = v0 ? d_v0 : nullptr; a.a0 = a0 ? d_a0 : nullptr;
  a.P0 = d_P0_.get(); a.per_target_P0 = per_target_P0 ? 1 : 0;
  a.cls = d_cls_.get(); a.cls_value = cls;
  if (cls_of || P0_index) {   // per-entry class / initial-covariance indices: behind the slot list in the index staging
    if (cls_of) { TE_HIP_CHECK(hipMemcpyAsync(d_idx_.get() + count, cls_of, sizeof(int) * count, hipMemcpyHostToDevice, stream_)); a.cls_of = d_idx_.get() + count; }
    if (P0_index) { TE_HIP_CHECK(hipMemcpyAsync(d_idx_.get() + 2 * count, P0_index, sizeof(int) * count, hipMemcpyHostToDevice, stream_)); a.P0_index = d_idx_.get() + 2 * count; }
  }
  a.t_off = te_clock_sub(t0, t_acc_); a.nm_off = (int)(-nm_acc_);
  a.t_base = d_tbase_.get(); a.nm_base = d_nmbase_.get();
  ops_->init(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipMemsetAsync(d_run_.get() + first, 0, (size_t)count, stream_));   // a new target has no rejections behind it
  TE_HIP_CHECK(hipMemsetAsync(d_miss_.get() + first, 0, (size_t)count, stream_));  // ... and neither misses nor hits
  TE_HIP_CHECK(hipMemsetAsync(d_hits_.get() + first, 0, (size_t)count, stream_));
  p0idx_dirty_.mark(first, count);
  if (d_gate_ring_) { if (gate_cap_ < cap_) gate_reserve(gate_window_); gate_reset(first, count); }
  if (keep_meas_) {
    init_measured_rows_kernel<<<(unsigned)((count * 7 + 255) / 256), 256, 0, stream_>>>(d_lastmeas_.get(), first, count);
    TE_HIP_CHECK(hipGetLastError());
  }
  if (p0_kept_ && bookkeeping) {   // host mirror of the initial covariances (initial_covariance)
    slot_p0_.resize((size_t)first, 0);
    if (P0_index) {
      std::vector<int> row((size_t)P0_count);
      for (long k = 0; k < P0_count && p0_kept_; ++k) row[(size_t)k] = intern_p0(P0 + (size_t)k * N * N);
      for (long i = 0; i < count && p0_kept_; ++i) slot_p0_.push_back(row[(size_t)P0_index[i]]);
    } else if (per_target_P0) {
      for (long i = 0; i < count && p0_kept_; ++i) { const int r = intern_p0(P0 + (size_t)i * N * N); if (p0_kept_) slot_p0_.push_back(r); }
    } else {
      const int r = intern_p0(P0);
      if (p0_kept_) slot_p0_.insert(slot_p0_.end(), (size_t)count, r);
    }
  }
  TE_HIP_CHECK(hipStreamSynchronize(stream_));  // host staging arrays may be pageable
  if (bookkeeping) {
    slot_ids_.insert(slot_ids_.end(), ids, ids + count);
    n_ += count;
  }
  return first;
}

long Batch::append_gathered(long count, const unsigned* ids, double t0, const double* P0, int cls, const double* det_dev, const int* rows_dev) {
  if (count > 0 && shared_axes() && !shared_axes_p0_ok(type_, P0, 1)) demote_shared();
  touch();
  if (count <= 0) return n_;
  return append_now(n_, count, ids, t0, P0, false, nullptr, nullptr, nullptr, cls, nullptr, nullptr, 0, true, det_dev, rows_dev);
}

unsigned Batch::erase_slot(long slot) {
  touch();
  const long last = n_ - 1;
  unsigned moved = slot_ids_[(size_t)slot];
  if (slot != last) {
    ops_->move_record(records(), last, slot, d_tbase_.get(), d_nmbase_.get(), d_cls_.get(), stream_);
    TE_HIP_CHECK(hipGetLastError());
    gate_move(last, slot);
    run_move(last, slot);
    if (d_lastmeas_) TE_HIP_CHECK(hipMemcpyAsync(d_lastmeas_.get() + 7 * slot, d_lastmeas_.get() + 7 * last, sizeof(double) * 7, hipMemcpyDeviceToDevice, stream_));
    if (p0_kept_) slot_p0_[(size_t)slot] = slot_p0_[(size_t)last];
    moved = slot_ids_[(size_t)last];
    slot_ids_[(size_t)slot] = moved;
  }
  if (p0_kept_) slot_p0_.pop_back();
  slot_ids_.pop_back();
  n_ = last;
  return moved;
}

void Batch::erase_slots(const int* slots, long k, std::vector<std::pair<unsigned, int>>& moves_out) {
  touch();
  moves_out.clear();
  if (k <= 0) return;
  const long new_n = n_ - k;
  std::vector<unsigned char> gone((size_t)n_, 0);
  for (long j = 0; j < k; ++j) {
    if (slots[j] < 0 || slots[j] >= n_ || gone[(size_t)slots[j]]) throw std::runtime_error("target_estimation_amd: erase_slots: bad or repeated slot");
    gone[(size_t)slots[j]] = 1;
  }
  // holes below the new size are filled, in order, by the survivors at or above it
  std::vector<int> src, dst;
  long tail = new_n;
  for (long hole = 0; hole < new_n; ++hole) {
    if (!gone[(size_t)hole]) continue;
    while (gone[(size_t)tail]) ++tail;
    src.push_back((int)tail); dst.push_back((int)hole);
    ++tail;
  }
  const long m = (long)src.size();
  if (m > 0) {
    stage_reserve(2 * m);
    TE_HIP_CHECK(hipMemcpyAsync(d_idx_.get(), src.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(d_idx_.get() + m, dst.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, stream_));
    ops_->move_records(records(), d_idx_.get(), d_idx_.get() + m, m, d_tbase_.get(), d_nmbase_.get(), d_cls_.get(), stream_);
    TE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(run_moves_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream_, d_run_.get(), d_idx_.get(), d_idx_.get() + m, m);
    TE_HIP_CHECK(hipGetLastError());
    launch_lifecycle_moves(d_miss_.get(), d_hits_.get(), d_idx_.get(), d_idx_.get() + m, m, stream_);
    for (long j = 0; j < m; ++j) {
      p0idx_dirty_.mark(dst[(size_t)j], 1);
      gate_move(src[(size_t)j], dst[(size_t)j]);
      if (d_lastmeas_) TE_HIP_CHECK(hipMemcpyAsync(d_lastmeas_.get() + 7 * (long)dst[(size_t)j], d_lastmeas_.get() + 7 * (long)src[(size_t)j], sizeof(double) * 7, hipMemcpyDeviceToDevice, stream_));
      if (p0_kept_) slot_p0_[(size_t)dst[(size_t)j]] = slot_p0_[(size_t)src[(size_t)j]];
      const unsigned id = slot_ids_[(size_t)src[(size_t)j]];
      slot_ids_[(size_t)dst[(size_t)j]] = id;
      moves_out.emplace_back(id, dst[(size_t)j]);
    }
    TE_HIP_CHECK(hipStreamSynchronize(stream_));   // src / dst go out of scope
  }
  slot_ids_.resize((size_t)new_n);
  if (p0_kept_) slot_p0_.resize((size_t)new_n);
  n_ = new_n;
}

void Batch::step_dense(double dt, const void* meas_dev, long ld, const unsigned char* has_dev) {
  touch();
  if (n_ == 0) return;
  StepParams p = dense_params();
  p.meas = meas_dev; p.meas_ld = ld; p.has_meas = has_dev; p.dt = dt;
  p.reverse = (flip_ && zigzag()) ? 1 : 0;   // zig-zag: consecutive dense ticks walk the tiles in opposite directions
  flip_ = !flip_;
  if (pingpong()) p.rec_out = alt_records();
  launch_step(p, stream_, host_meas_rows_);
  if (p.rec_out) swap_records();   // later launches on the stream see the finished tick in the new current buffer
  t_acc_ = te_clock_add(t_acc_, dt);
  if (meas_dev && !has_dev) nm_acc_ += 1;
}

void Batch::check_pose_stream(const PoseStream& q) const {
  if (!q.dev) return;
  if (q.ld < n_) throw std::invalid_argument("target_estimation_amd: pose stream: ld " + std::to_string(q.ld) + " < batch size " + std::to_string(n_));
  if (q.tick_stride < 0 || (q.tick_stride > 0 && q.tick_stride < 7 * q.ld))
    throw std::invalid_argument("target_estimation_amd: pose stream: tick_stride must be 0 or >= 7 * ld");
  if (q.ring < 0) throw std::invalid_argument("target_estimation_amd: pose stream: negative ring_ticks");
}

void Batch::check_innov_stream(const InnovStream& q, bool count_only_needs_no_p0) const {
  const bool p0_kept_ = this->p0_kept_ || (count_only_needs_no_p0 && q.reacq.on && q.reacq.k == 0);   // (K = 0 never reads a P0)
  if (!(q.gate >= 0.0)) throw std::invalid_argument("target_estimation_amd: gate: nis_max must be 0 (no gate) or positive");
  if (q.gated() && !q.nis) throw std::invalid_argument("target_estimation_amd: gate: nis_max > 0 needs an innovation stream with a NIS row (it reports the decisions)");
  if (!q.nis) { check_reacquire(q.reacq, q.gate, n_, keep_meas_, p0_kept_); return; }
  const long m = ops_->L.m;
  if (q.ld < n_) throw std::invalid_argument("target_estimation_amd: innovation stream: ld " + std::to_string(q.ld) + " < batch size " + std::to_string(n_));
  if (q.nis_tick_stride < 0 || (q.nis_tick_stride > 0 && q.nis_tick_stride < q.ld))
    throw std::invalid_argument("target_estimation_amd: innovation stream: nis_tick_stride must be 0 or >= ld");
  if (q.innov_tick_stride < 0 || (q.innov_tick_stride > 0 && q.innov_tick_stride < m * q.ld))
    throw std::invalid_argument("target_estimation_amd: innovation stream: innov_tick_stride must be 0 or >= " + std::to_string(m) + " * ld");
  if (q.ring < 0) throw std::invalid_argument("target_estimation_amd: innovation stream: negative ring_ticks");
  check_reacquire(q.reacq, q.gate, n_, keep_meas_, p0_kept_);
}

void Batch::step_sequence(long n_ticks, double dt, const void* meas_base, long tick_stride, long ld,
                          const unsigned char* has_base, long has_stride, int use_graph, long ring_ticks, const PoseStream& poses,
                          const InnovStream& innov, const DtSchedule& sched) {
  check_pose_stream(poses);   // (before touch(): a refused call launches nothing)
  check_innov_stream(innov);
  if (sched.on() && sched.n != n_ticks) throw std::invalid_argument("target_estimation_amd: the time-step schedule has one entry per tick of the call");
  touch();
  if (n_ == 0 || n_ticks <= 0) return;
  prepare_reacquire(innov);   // (before anything is enqueued or recorded)
  const SeqSpec q{meas_base, tick_stride, ld, has_base, has_stride, nullptr, nullptr, ring_ticks, poses, innov};
  auto tick = [&](hipStream_t st, long s, bool ab) {
    const bool reverse = zigzag() && ((s + (use_graph ? 0 : (flip_ ? 1 : 0))) & 1) != 0;   // zig-zag; a recorded graph starts forwards
    enqueue_tick(st, s, sched.at(s, dt), q, false, nullptr, 0.0, reverse, ab);
  };
  if (!use_graph) {
    const bool ab = pingpong() && !innov.on();   // (a tick with an innovation stream runs in place: same bits)
    for (long s = 0; s < n_ticks; ++s) tick(stream_, s, ab);
    TE_HIP_CHECK(hipGetLastError());
    if (n_ticks & 1) flip_ = !flip_;
  } else {
    auto* hit = graphs_.find([&](const SeqKey& k) { return k.n_ticks == n_ticks && k.n == n_ && k.rec == d_rec_.get() && k.dt.matches(sched, dt) && k.spec.same(q); });
    if (!hit) {   // (full, e.g. a ring of 4096 ticks replayed in 64-tick blocks: the least recently used recording goes)
      if (!cap_stream_) TE_HIP_CHECK(hipStreamCreateWithFlags(cap_stream_.out(), hipStreamNonBlocking));
      hit = &graphs_.record(SeqKey{n_ticks, n_, d_rec_.get(), q, DtKey(sched, dt)}, stream_, cap_stream_.get(), [&] {
        const RecordingScope recording(*this);
        for (long s = 0; s < n_ticks; ++s) {
          tick(cap_stream_.get(), s, false);
#ifdef TE_TEST_HOOKS   // only in libtarget_estimation_amd_testhooks.so (csrc/Makefile `testhooks`)
          if (s == 0 && std::getenv("TE_TEST_FAIL_IN_CAPTURE"))   // test hook: a launch that throws between Begin and EndCapture
            throw std::runtime_error("target_estimation_amd: injected failure inside stream capture");
#endif
        }
        TE_HIP_CHECK(hipGetLastError());
      });
    }
    graphs_.stamp(*hit);
    if (use_graph == 2) return;  // record only
    TE_HIP_CHECK(hipGraphLaunch(hit->exec.get(), stream_));
    note_replay(n_ticks);
    flip_ = (n_ticks & 1) != 0;   // the graph's last tick ran forwards (odd count) or backwards
  }
  account(n_ticks, dt, sched, q.all_measured());
}

StepParams Batch::tick_params(long s, double dt, const SeqSpec& q, bool query, const double* origin, double radius, bool ab) {
  const long sm = q.ring_ticks > 0 ? s % q.ring_ticks : s;   // the measurements' ring; the streams have their own: tick s of the call
  StepParams p = dense_params();
  p.pose = q.poses.block(s); p.pose_ld = q.poses.ld;
  p.nis = q.innov.nis_row(s); p.innov = q.innov.innov_block(s); p.innov_ld = q.innov.ld; p.gate = q.innov.gate;
  p.meas = q.meas_base ? static_cast<const char*>(q.meas_base) + (size_t)(sm * q.tick_stride) * elem_size() : nullptr;
  p.meas_ld = q.ld;
  p.has_meas = q.has_base ? q.has_base + sm * q.has_stride : nullptr;
  p.dt = dt;
  if (query) {
    p.q_origin[0] = origin[0]; p.q_origin[1] = origin[1]; p.q_origin[2] = origin[2];
    p.q_radius = radius; p.q_delta = q.delta_dev; p.q_pose = q.pose_dev;
  }
  if (ab && !p.q_delta) p.rec_out = alt_records();   // (the fused query's kernels have no A -> B form: in place)
  return p;
}

void Batch::enqueue_tick(hipStream_t st, long s, double dt, const SeqSpec& q, bool query, const double* origin, double radius,
                         bool reverse, bool ab) {
  if (n_ == 0) return;
  // (a tick with an innovation stream runs in place and without the fused query: the query follows as intersect_kernel)
  const bool fused_q = query && n_classes_ == 1 && !q.innov.on();
  StepParams p = tick_params(s, dt, q, fused_q, origin, radius, ab && !q.innov.on());
  fill_reacquire(p, q.innov, s);
  p.reverse = reverse ? 1 : 0;
  launch_step(p, st);
  if (p.rec_out) swap_records();
  if (query && !fused_q) enqueue_own_time_query(st, q, origin, radius);
}

void Batch::enqueue_own_time_query(hipStream_t st, const SeqSpec& q, const double* origin, double radius) {
  IntersectArgs a;
  a.rec = records_as_stored(); a.idx = nullptr; a.n = n_; a.t1 = std::numeric_limits<double>::quiet_NaN();
  a.origin[0] = origin[0]; a.origin[1] = origin[1]; a.origin[2] = origin[2]; a.radius = radius;
  a.t_acc = TClock{0.0, 0.0}; a.t_base = d_tbase_.get(); a.delta = q.delta_dev; a.pose = q.pose_dev;
  ops_->intersect(a, st);
}

bool Batch::population_ready() const {
  return ops_->L.layout == LAYOUT_SEPARABLE_PACKED && n_classes_ == 1 && !keep_meas_;
}

void Batch::enqueue_after_innov_tick(hipStream_t st, long s, const SeqSpec& q, bool query, const double* origin, double radius) {
  if (n_ == 0) return;
  if (q.innov.reacq.on && q.meas_base) {   // behind the population tick's step, ahead of the poses and the query
    const long sm = q.ring_ticks > 0 ? s % q.ring_ticks : s;
    StepParams p;
    p.rec = records_as_stored(); p.n = n_;
    p.meas = static_cast<const char*>(q.meas_base) + (size_t)(sm * q.tick_stride) * elem_size(); p.meas_ld = q.ld;
    p.has_meas = q.has_base ? q.has_base + sm * q.has_stride : nullptr;
    p.nis = q.innov.nis_row(s); p.gate = q.innov.gate;
    if (uniform_tiles_enabled() && d_tile_uni_) { p.tile_blk = d_tile_blk_.get(); p.tile_uni = d_tile_uni_.get(); }
    fill_reacquire(p, q.innov, s);
    ops_->reacquire(make_reacquire_args(p), st);
  }
  if (q.poses.dev) {
    OutArgs o;
    o.rec = records_as_stored(); o.idx = nullptr; o.n = n_; o.pose = nullptr; o.twist = nullptr; o.acc = nullptr;
    o.at_time = 0; o.t1 = 0.0; o.t_acc = TClock{0.0, 0.0}; o.t_base = d_tbase_.get();
    o.pose_soa = q.poses.block(s); o.pose_ld = q.poses.ld;
    ops_->outputs(o, st);
  }
  if (query) enqueue_own_time_query(st, q, origin, radius);
}

void Batch::account(long n_ticks, double dt, const DtSchedule& sched, bool all_measured) {
  t_acc_ = sched.on() ? sched.advance(t_acc_) : te_clock_add_ticks(t_acc_, dt, (double)n_ticks);
  if (all_measured) nm_acc_ += n_ticks;
}

const double* Batch::dt_table_push(const double* dt_host, long n) { return dttab_.push(dt_host, n, stream_); }

void Batch::step_fused(long n_ticks, double dt, const void* meas_base, long tick_stride, long ld,
                       const unsigned char* has_base, long has_stride, const PoseStream& poses, const DtSchedule& sched) {
  step_fused_gated(n_ticks, dt, meas_base, tick_stride, ld, has_base, has_stride, poses, InnovStream{}, sched);
}

void Batch::check_fused_call(long n_ticks, const SeqSpec& q, const DtSchedule& sched, bool one_launch) const {
  if (sched.on() && sched.n != n_ticks) throw std::invalid_argument("target_estimation_amd: the time-step schedule has one entry per tick of the call");
  check_pose_stream(q.poses);   // (before touch(): a refused call launches nothing)
  check_innov_stream(q.innov, one_launch);   // (the kernel's K = 0 reads no initial covariance; the single ticks' launch is given the table)
  if (n_ticks > 0x7fffffffL) throw std::invalid_argument("target_estimation_amd: step_fused_gated: n_ticks does not fit an int");
  if (q.tick_stride < 0 || q.has_stride < 0) throw std::invalid_argument("target_estimation_amd: step_fused_gated: negative stride");
  if (q.meas_base && q.ld < n_) throw std::invalid_argument("target_estimation_amd: step_fused_gated: ld " + std::to_string(q.ld) + " < batch size " + std::to_string(n_));
}

bool Batch::fused_call_one_launch(const SeqSpec& q, const DtSchedule& sched) const {
  return (sched.on() ? fused_dt_served(!q.innov.plain()) : fused_gate_served()) && !q.poses.dev;
}

void Batch::fused_call_begin(const SeqSpec& q) {
  touch();
  demote_shared();   // (the temporally fused kernels exist for the plain form only)
  if (n_ > 0) prepare_fused_reacquire(q.innov);
}

void Batch::prepare_fused_reacquire(const InnovStream& innov) {
  if (innov.reacq.on && (innov.reacq.k > 0 || p0_kept_)) prepare_p0_tables();   // (before anything is enqueued)
}

StepParams Batch::fused_call_params(long n_ticks, double dt, const SeqSpec& q, const DtSchedule& sched, const double* dt_tab) {
  const InnovStream& innov = q.innov;
  StepParams p = base_params();
  p.gate_row = d_has_eff_.get();   // (the dense layouts' single gated ticks take their mask from the writer's row)
  p.meas = q.meas_base; p.meas_ld = q.ld; p.has_meas = q.has_base; p.dt = dt;
  p.n_ticks = (int)n_ticks; p.tick_stride = q.tick_stride; p.has_stride = q.has_stride;
  p.pose = q.poses.dev; p.pose_ld = q.poses.ld; p.pose_tick_stride = q.poses.tick_stride; p.pose_ring = q.poses.ring;
  if (!innov.plain()) {   // (plain: no stream, no gate -- the plain fused loop)
    p.fused_gate = 1; p.fused_gate_nis_max = innov.gate;
    p.fused_gate_nis = innov.nis; p.fused_gate_nis_stride = innov.nis_tick_stride; p.fused_gate_nis_ring = innov.ring;
    p.fused_gate_innov = innov.innov; p.fused_gate_innov_ld = innov.ld; p.fused_gate_innov_stride = innov.innov_tick_stride;
    if (innov.reacq.on) {
      p.fused_gate_k = innov.reacq.k; p.reacq_run = d_run_.get(); p.reacq_p0 = d_p0tab_.get(); p.reacq_p0_idx = d_p0idx_.get();
      p.fused_gate_event = innov.reacq.event; p.fused_gate_event_stride = innov.reacq.tick_stride; p.fused_gate_event_ring = innov.reacq.ring;
    }
  }
  if (sched.on()) { p.dt_sched = 1; p.dt_host = sched.dt; p.dt = 0.0; p.dt_tab = dt_tab; }
  return p;
}

void Batch::step_fused_gated(long n_ticks, double dt, const void* meas_base, long tick_stride, long ld, const unsigned char* has_base,
                             long has_stride, const PoseStream& poses, const InnovStream& innov, const DtSchedule& sched) {
  const SeqSpec q{meas_base, tick_stride, ld, has_base, has_stride, nullptr, nullptr, 0, poses, innov};
  const bool fused_only = innov.plain() && !sched.on();   // step_fused as it always was: its refusals are the pose stream's
  if (fused_only) check_pose_stream(poses);
  else check_fused_call(n_ticks, q, sched, fused_call_one_launch(q, sched));
  touch();
  demote_shared();   // (the temporally fused kernels exist for the plain form only)
  if (n_ == 0 || n_ticks <= 0) return;
  // measured-pose rows keep ACCEPTED measurements, tick by tick: the sequence's launches.  So does a schedule beyond what one
  // table's 32-bit byte offsets reach (kDtTabMaxTicks).
  if (!fused_only && (keep_meas_ || (sched.on() && n_ticks > kDtTabMaxTicks))) {
    step_sequence(n_ticks, dt, meas_base, tick_stride, ld, has_base, has_stride, 0, 0, poses, innov, sched);
    return;
  }
  prepare_fused_reacquire(innov);
  // the table: a run of the batch's ring that no other call shares, filled on the stream ahead of the launch
  launch_step(fused_call_params(n_ticks, dt, q, sched, sched.on() ? dt_table_push(sched.dt, n_ticks) : nullptr), stream_);
  TE_HIP_CHECK(hipGetLastError());
  account(n_ticks, dt, sched, q.all_measured());
}

// device block of a live session: [one mirror word per kLiveGroup wavefronts, 128 bytes apart][progress words]
static size_t live_mirror_bytes(long waves) { return (size_t)((waves + kLiveGroup - 1) / kLiveGroup) * kLiveMirrorStride * sizeof(long long); }
static long live_progress_words(long waves) { return (waves + kLiveScan - 1) / kLiveScan * kLiveScan; }   // whole relay scans
static size_t live_block_bytes(long waves) { return (live_mirror_bytes(waves) + sizeof(int) * (size_t)live_progress_words(waves) + 15) / 16 * 16; }

void Batch::live_start(double dt, const void* meas_ring, long tick_stride, long ld, const unsigned char* has_ring, long has_stride,
                       long ring_ticks, long first_entry, long max_ticks, double idle_limit_s, const double* q_origin, double q_radius,
                       double* q_delta_dev, double* q_pose_dev) {
  touch();   // ends a previous session, runs queued one-target steps
  demote_shared();   // the resident kernels hold plain records (before the session exists: this frees device memory)
  if (q_delta_dev && !q_origin) throw std::invalid_argument("target_estimation_amd: live_start: query without an origin");
  if (n_ == 0) throw std::runtime_error("target_estimation_amd: live mode on an empty batch");
  if (!meas_ring || ring_ticks <= 0 || max_ticks <= 0 || first_entry < 0 || ld < n_ || tick_stride < 7 * ld || (has_ring && has_stride < n_))
    throw std::invalid_argument("target_estimation_amd: live_start: bad measurement ring");
  if (max_ticks > 0x7fffffffL) throw std::invalid_argument("target_estimation_amd: live_start: at most 2^31 - 1 ticks per session");
  if (n_classes_ > 1) throw std::runtime_error("target_estimation_amd: live mode serves batches with one (Q, R) class");
  const InnovStream& lgate = live_.gate;
  if (lgate.gated()) {   // (what may have changed since live_set_gate)
    if (const char* why = live_gate_refusal()) throw std::runtime_error(why);
    if (lgate.ld < n_ || (lgate.reacq.event && lgate.reacq.ld < n_))
      throw std::invalid_argument("target_estimation_amd: live gate: rows shorter than the batch (it grew since live_set_gate)");
    if (lgate.reacq.on && lgate.reacq.k > 0) prepare_p0_tables();   // (throws if the batch no longer keeps its initial covariances)
  }
  long cap = ops_->live_capacity ? ops_->live_capacity(live_kernel_next(q_delta_dev != nullptr)) : 0;
  if (const char* e = std::getenv("TE_LIVE_CAPACITY_WAVES")) { if (cap > 0 && std::atol(e) > 0) cap = std::atol(e); }   // experiments only (tools/live_capacity.py --probe)
  if (cap <= 0) throw std::runtime_error("target_estimation_amd: live mode needs the axis-separable layout with packed groups");
  const long waves = (n_ + ops_->L.tpw - 1) / ops_->L.tpw;
  if (waves > cap)
    throw std::runtime_error("target_estimation_amd: live mode: " + std::to_string(n_) + " targets need " + std::to_string(waves) +
                             " resident wavefronts, the device holds " + std::to_string(cap) + " of this kernel");
  if (waves + 1 > cap) throw std::runtime_error("target_estimation_amd: live mode: no room for the relay wavefront");
  // ... and next to the sessions that are resident already (other batches, other managers of this process): their grids hold
  // their wave slots until they end, so a grid that only fits an empty device would start in part and never get its relay
  const double share = (double)(waves + 1) / (double)cap;
  if (!live_session_begin(share))
    throw std::runtime_error("target_estimation_amd: live mode: " + std::to_string(n_) + " targets take " + std::to_string((int)(share * 100.0 + 0.5)) +
                             " % of the device's resident wavefronts and the sessions already resident in this process take " +
                             std::to_string((int)(live_sessions_share() * 100.0 + 0.5)) + " %: they do not fit the device together");
  live_.share = share;   // counted from here on; every way out of the session gives it back (live_release)
  try {
  if (!live_.h_block) {
    live_.h_block.alloc(128, kPinnedMapped);
    char* const h = live_.h_block.host();
    char* const d = live_.h_block.dev();
    live_.h_posted = reinterpret_cast<long long*>(h); live_.d_posted = reinterpret_cast<long long*>(d);
    live_.h_done = reinterpret_cast<int*>(h + 64); live_.d_done = reinterpret_cast<int*>(d + 64);
    // The doorbell itself lives in DEVICE memory where the host can write it through the PCIe BAR (large-BAR systems, fine-grained
    // device memory: the device pointer is valid on the host): the relay then polls a local word instead of reading host memory
    // over PCIe every round -- the direction that costs a round trip (tools/bar_doorbell.hip: 2.66 -> 2.21 us per echo).  The
    // completion word stays in host memory: the GPU writes it, the host polls its own memory.  TE_LIVE_DOORBELL=host keeps both there.
    const char* e = std::getenv("TE_LIVE_DOORBELL");
    int dev = 0, large_bar = 0;
    if (!(e && e[0] == 'h') && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) == hipSuccess && large_bar) {
      if (live_.bar_bell.try_alloc_finegrained(128 / sizeof(long long))) live_.h_posted = live_.d_posted = live_.bar_bell.get();
    }
  }
  if (waves > live_.cap_waves) {
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    live_.cap_waves = 0;
    live_.d_block.alloc(live_block_bytes(waves));
    live_.cap_waves = waves;
  }
  __atomic_store_n(live_.h_posted, 0LL, __ATOMIC_RELAXED);
  __atomic_store_n(live_.h_done, -1, __ATOMIC_RELAXED);   // the relay's first store makes it 0: "running"
  __atomic_store_n(live_.h_done + 2, 0, __ATOMIC_RELAXED);    // the relay's last store makes it 1: "ended"
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  // The resident kernel gets a stream of its own (non-blocking), ordered behind everything already queued on the batch's
  // stream: nothing the caller queues later on that stream -- for this batch's siblings in the manager, say -- waits for the
  // session, and two batches of one manager can be resident together.
  if (!live_.stream) {
    // A stream of its own PRIORITY class: the runtime multiplexes the streams of one priority over a few hardware queues, and
    // a stream that lands in the resident kernel's queue waits until the session ends (a ring refill on "another stream" took
    // 1.6 - 17 s, i.e. the idle limit, whenever that happened; with GPU_MAX_HW_QUEUES=1 always).  Queues are not shared across
    // priorities, so the resident kernel gets the high-priority class to itself (callers' streams are normal priority unless
    // they ask otherwise).
    int least = 0, greatest = 0;
    TE_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (const char* e = std::getenv("TE_LIVE_STREAM_PRIORITY")) {   // experiments only (tools/r4_regress.sh): 0 = normal, low = least
      if (e[0] == 'l') greatest = least; else if (std::atoi(e) == 0) greatest = 0;
    }
    TE_HIP_CHECK(hipStreamCreateWithPriority(live_.stream.out(), hipStreamNonBlocking, greatest));
  }
  if (!live_.ready) TE_HIP_CHECK(hipEventCreateWithFlags(live_.ready.out(), hipEventDisableTiming));
  TE_HIP_CHECK(hipEventRecord(live_.ready.get(), stream_));
  TE_HIP_CHECK(hipStreamWaitEvent(live_.stream.get(), live_.ready.get(), 0));
  TE_HIP_CHECK(hipMemsetAsync(live_.d_block.get(), 0, live_block_bytes(waves), live_.stream.get()));   // mirrors + progress: zero before EVERY launch
  if (live_progress_words(waves) > waves)   // the padding of the progress words: INT_MAX, neutral in the relay's minimum
    TE_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(live_.d_block.get() + live_mirror_bytes(waves) + sizeof(int) * (size_t)waves), 0x7fffffff,
                                   (size_t)(live_progress_words(waves) - waves), live_.stream.get()));
  StepParams p = base_params();
  p.meas = meas_ring; p.meas_ld = ld; p.has_meas = has_ring; p.dt = dt;
  p.n_ticks = (int)max_ticks; p.tick_stride = tick_stride; p.has_stride = has_stride;
  p.live_posted = live_.d_posted; p.live_done = live_.d_done;
  p.live_mirror = reinterpret_cast<long long*>(live_.d_block.get()); p.live_progress = reinterpret_cast<int*>(live_.d_block.get() + live_mirror_bytes(waves));
  p.live_ring = ring_ticks; p.live_first = first_entry % ring_ticks;
  // a poll is a PCIe round trip plus s_sleep: ~1-2 us; the limit is a count of polls
  const double polls = idle_limit_s > 0 ? idle_limit_s * 5e5 : 5e6;
  p.live_spin_limit = (unsigned)std::min(polls, 4.0e9);
  {   // the relay measures the idle time on the device's constant-rate clock; the count above bounds the workers' own spins
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0)
      p.live_idle_ticks = (unsigned long long)((idle_limit_s > 0 ? idle_limit_s : 10.0) * 1e3 * (double)khz);
  }
  { const char* e = std::getenv("TE_LIVE_FLAGS"); p.live_flags = e ? std::atoi(e) : 0; }
  if (live_.pose_out) {
    if (live_.pose_ld < n_) throw std::invalid_argument("target_estimation_amd: live pose output: rows shorter than the batch (it grew since live_set_pose_output)");
    p.live_pose = live_.pose_out; p.live_pose_ld = live_.pose_ld;
  }
  if (q_delta_dev) {
    p.q_origin[0] = q_origin[0]; p.q_origin[1] = q_origin[1]; p.q_origin[2] = q_origin[2];
    p.q_radius = q_radius; p.q_delta = q_delta_dev; p.q_pose = q_pose_dev;
  }
  if (lgate.gated()) {
    p.live_gate = 1; p.live_gate_nis_max = lgate.gate;
    p.live_gate_nis = lgate.nis; p.live_gate_nis_stride = lgate.nis_tick_stride; p.live_gate_nis_ring = lgate.ring;
    p.live_gate_k = lgate.reacq.on ? lgate.reacq.k : -1;
    if (lgate.reacq.on) {
      p.reacq_run = d_run_.get(); p.reacq_p0 = d_p0tab_.get(); p.reacq_p0_idx = d_p0idx_.get();
      p.live_gate_event = lgate.reacq.event; p.live_gate_event_stride = lgate.reacq.tick_stride; p.live_gate_event_ring = lgate.reacq.ring;
    }
  }
  ops_->step(p, live_.stream.get());   // (the measured-pose rows are not kept during a live session: see measured_pose.hpp)
  TE_HIP_CHECK(hipGetLastError());
  live_.waves = waves; live_.posted = 0; live_.max_ticks = max_ticks; live_.dt = dt;
  live_.all_measured = has_ring == nullptr && !lgate.gated();   // (a gated session counts its accepted measurements per slot)
  // The session exists once its LAST workgroup (the relay) says so: then every worker holds its wave slot.  A kernel that is
  // still queued after two seconds is not going to run next to whatever is ahead of it (its stream shares a hardware queue with
  // another endless kernel -- more live batches than GPU_MAX_HW_QUEUES, or a caller's own high-priority stream -- or the device
  // cannot hold the whole grid): told to stop as soon as it starts, and reported, instead of a session that never serves a tick.
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::duration<double>(kLiveStartTimeoutS);
  for (unsigned spins = 0; __atomic_load_n(live_.h_done, __ATOMIC_ACQUIRE) < 0; ++spins) {
    __builtin_ia32_pause();
    if ((spins & 1023u) != 1023u) continue;
    const hipError_t q = hipStreamQuery(live_.stream.get());
    if (q != hipErrorNotReady && q != hipSuccess) TE_HIP_CHECK(q);
    if (std::chrono::steady_clock::now() < t_end) continue;
    __atomic_store_n(live_.h_posted, kLiveStop, __ATOMIC_RELEASE);
    if (live_.bar_bell) __builtin_ia32_sfence();
    // (workers that did get a wave slot look at the host's word themselves every millisecond or two: they leave, the rest of the
    // grid gets their slots, sees the stop and leaves too; the records are back as they were)
    const auto t_gone = std::chrono::steady_clock::now() + std::chrono::duration<double>(1.0);
    while (hipStreamQuery(live_.stream.get()) == hipErrorNotReady && std::chrono::steady_clock::now() < t_gone) __builtin_ia32_pause();
    live_.zombie = hipStreamQuery(live_.stream.get()) == hipErrorNotReady;   // still queued behind somebody else's kernel: flush() waits for it before anything touches the records
    if (!live_.zombie) live_release();
    throw std::runtime_error("target_estimation_amd: live mode: the resident kernel did not start within " + std::to_string(kLiveStartTimeoutS) +
                             " s (its stream shares a hardware queue with another endless kernel -- more live batches than GPU_MAX_HW_QUEUES, or a "
                             "high-priority stream of the caller -- or the device is busy)");
  }
  } catch (...) {
    if (!live_.zombie) live_release();   // (a zombie still holds its place: flush() releases it once the kernel is gone)
    throw;
  }
  live_.active = true;
}

void Batch::live_release() {
  if (live_.share > 0.0) { const double s = live_.share; live_.share = 0.0; live_session_ended(s); }
}

void Batch::live_set_pose_output(double* pose_soa_dev, long ld) {
  if (pose_soa_dev && ld < n_) throw std::invalid_argument("target_estimation_amd: live pose output: rows shorter than the batch");
  live_.pose_out = pose_soa_dev;
  live_.pose_ld = pose_soa_dev ? ld : 0;
}

const char* Batch::live_gate_refusal() const {
  const Ops* o = shared_axes() ? get_ops(type_, dtype_, lanes_code_) : ops_;
  if (!o || !o->live_capacity || o->L.layout != LAYOUT_SEPARABLE_PACKED)
    return "target_estimation_amd: live gate: no gated resident kernel for this batch (live mode needs the axis-separable layout with packed groups)";
  if (n_classes_ > 1) return "target_estimation_amd: live gate: live mode serves batches with one (Q, R) class";
  if (keep_meas_) return "target_estimation_amd: live gate: not served for a batch that keeps measured poses (set_keep_measurement)";
  return nullptr;
}

void Batch::live_set_gate(const InnovStream& g) {
  const std::string pre = "target_estimation_amd: live gate: ";
  if (!(g.gate >= 0.0)) throw std::invalid_argument(pre + "nis_max must be 0 (no gate) or positive");
  if (!g.gated()) {
    if (g.reacq.on) throw std::invalid_argument(pre + "a policy needs the gate (nis_max > 0): it counts the gate's rejections");
    touch();   // (a session that runs keeps the gate it started with; the next one has none)
    live_.gate = InnovStream{};
    return;
  }
  if (!g.nis) throw std::invalid_argument(pre + "nis_max > 0 needs the NIS rows of the session (nis_dev): they report the decisions");
  if (g.innov) throw std::invalid_argument(pre + "the innovations are not served in resident sessions (innov_dev must be NULL)");
  if (g.ld < n_) throw std::invalid_argument(pre + "ld " + std::to_string(g.ld) + " < batch size " + std::to_string(n_));
  if (g.nis_tick_stride < 0 || (g.nis_tick_stride > 0 && g.nis_tick_stride < g.ld)) throw std::invalid_argument(pre + "nis_tick_stride must be 0 or >= ld");
  if (g.ring < 0) throw std::invalid_argument(pre + "negative ring_ticks");
  if (g.reacq.on) {
    if (g.reacq.k < 0 || g.reacq.k > 127) throw std::invalid_argument(pre + "max_rejects must be 0..127, got " + std::to_string(g.reacq.k));
    if (g.reacq.event) {
      if (g.reacq.ld < n_) throw std::invalid_argument(pre + "event rows: ld " + std::to_string(g.reacq.ld) + " < batch size " + std::to_string(n_));
      if (g.reacq.tick_stride < 0 || (g.reacq.tick_stride > 0 && g.reacq.tick_stride < g.reacq.ld)) throw std::invalid_argument(pre + "event rows: tick_stride must be 0 or >= ld");
      if (g.reacq.ring < 0) throw std::invalid_argument(pre + "event rows: negative ring_ticks");
    }
    if (g.reacq.k > 0 && !p0_kept_) throw std::invalid_argument(pre + "max_rejects > 0: the batch no longer keeps its initial covariances (too many distinct ones)");
  }
  if (const char* why = live_gate_refusal()) throw std::runtime_error(why);
  touch();   // (ends a session that runs: it keeps the gate it started with)
  live_.gate = g;
}

void Batch::live_post(long n_ticks) {
  if (!live_.active) throw std::runtime_error("target_estimation_amd: live_post without a live session");
  if (n_ticks <= 0) return;
  if (live_.posted + n_ticks > live_.max_ticks) throw std::runtime_error("target_estimation_amd: live_post beyond the session's max_ticks");
  live_.posted += n_ticks;
  __atomic_store_n(live_.h_posted, (long long)live_.posted, __ATOMIC_RELEASE);   // the ring entries were written before this call
  if (live_.bar_bell) __builtin_ia32_sfence();   // (device memory behind the BAR is write-combined on the host: push the store out now)
}

long Batch::live_done() const {
  if (!live_.active) return 0;
  return std::max(0L, (long)__atomic_load_n(live_.h_done, __ATOMIC_ACQUIRE));
}

bool Batch::live_wait(long tick, double timeout_s) const {
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::duration<double>(timeout_s);
  for (unsigned spins = 0;; ++spins) {
    if (live_done() >= tick) return true;
    __builtin_ia32_pause();
    if ((spins & 255u) == 255u && std::chrono::steady_clock::now() >= t_end) return false;
  }
}

long Batch::live_stop() {
  if (!live_.active) return 0;
  __atomic_store_n(live_.h_posted, (long long)live_.posted | kLiveStop, __ATOMIC_RELEASE);
  if (live_.bar_bell) __builtin_ia32_sfence();
  live_.active = false;     // whatever happens below, the session is over (flush() must not come back here)
  {
    const hipError_t e = hipStreamSynchronize(live_.stream.get());   // bounded: every wavefront drains the posted ticks, then sees the stop bit
    live_release();                                          // the kernel is gone: its wave slots, and the frees that waited for it
    TE_HIP_CHECK(e);
  }
  // the relay's last word: the ticks EVERY wavefront served.  The host's stop, or the relay's own after a silent host, reaches
  // all workers through one device word, so they all stop at the same tick.
  const long mn = std::max(0L, (long)__atomic_load_n(live_.h_done, __ATOMIC_ACQUIRE));
  account(mn, live_.dt, DtSchedule{}, live_.all_measured);
  if (mn != live_.posted)
    throw std::runtime_error("target_estimation_amd: live session ended after " + std::to_string(mn) + " of " + std::to_string(live_.posted) +
                             " posted ticks (the idle limit stopped it before the last post?)");
  return (long)mn;
}

void Batch::step_indexed(const int* slots, long n, double dt, const double* meas_aos, const unsigned char* has, double* nis_out,
                         unsigned char* event_out) {
  touch();
  if (n <= 0) return;
  const bool pol = pol_.on() && meas_aos != nullptr;
  if (!pol) {   // (the plain kernels report nothing: no measurement was judged)
    if (nis_out) std::fill(nis_out, nis_out + n, -1.0);
    if (event_out) std::fill(event_out, event_out + n, (unsigned char)0);
  }
  stage_reserve(n);
  upload_slots(slots, n);
  if (meas_aos) {
    TE_HIP_CHECK(hipMemcpyAsync(d_aos_.get(), meas_aos, sizeof(double) * 7 * n, hipMemcpyHostToDevice, stream_));
    ops_->pack_meas(d_aos_.get(), n, d_meas_.get(), n, stream_);
  }
  if (has) TE_HIP_CHECK(hipMemcpyAsync(d_mask_.get(), has, (size_t)n, hipMemcpyHostToDevice, stream_));
  StepParams p = base_params();
  p.n = n; p.idx = d_idx_.get(); p.meas = meas_aos ? d_meas_.get() : nullptr; p.meas_ld = n;
  p.has_meas = (meas_aos && has) ? d_mask_.get() : nullptr; p.dt = dt;
  if (pol) fill_update_gate(p, n);
  launch_step(p, stream_);
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipStreamSynchronize(stream_));  // caller's host arrays may be reused after return
  if (pol) {
    if (nis_out) std::copy(pol_nis_host(), pol_nis_host() + n, nis_out);
    if (event_out) std::copy(pol_event_host(), pol_event_host() + n, event_out);
  }
}

void Batch::step_indexed_dev(const int* idx_dev, long n, double dt, const void* meas_soa_dev, long ld, const unsigned char* has_dev,
                             double* nis_dev, unsigned char* event_dev) {
  touch();
  if (n <= 0) return;
  StepParams p = base_params();
  p.n = n; p.idx = idx_dev; p.meas = meas_soa_dev; p.meas_ld = ld;
  p.has_meas = meas_soa_dev ? has_dev : nullptr; p.dt = dt;
  if (pol_.on() && meas_soa_dev) fill_update_gate(p, n, nis_dev, event_dev);
  launch_step(p, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::outputs_indexed_dev(const int* idx_dev, long n, double* pose_dev, double* twist_dev, double* acc_dev, bool at_time, double t1) {
  flush();
  if (n <= 0) return;
  OutArgs a;
  a.rec = records_as_stored(); a.idx = idx_dev; a.n = n; a.pose = pose_dev; a.twist = twist_dev; a.acc = acc_dev;
  a.at_time = at_time ? 1 : 0; a.t1 = t1; a.t_acc = t_acc_; a.t_base = d_tbase_.get();
  ops_->outputs(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::step_dense_host(double dt, const double* meas_aos, const unsigned char* has, double* nis_out, unsigned char* event_out) {
  touch();   // before the staging buffers are filled: a pending flush uses them too
  if (n_ == 0) return;
  const bool pol = pol_.on() && meas_aos != nullptr;
  if (!pol) {
    if (nis_out) std::fill(nis_out, nis_out + n_, -1.0);
    if (event_out) std::fill(event_out, event_out + n_, (unsigned char)0);
  } else if (const char* why = update_gate_refusal()) {
    throw std::runtime_error(why);
  }
  stage_reserve(n_);
  if (meas_aos) {
    TE_HIP_CHECK(hipMemcpyAsync(d_aos_.get(), meas_aos, sizeof(double) * 7 * n_, hipMemcpyHostToDevice, stream_));
    ops_->pack_meas(d_aos_.get(), n_, d_meas_.get(), n_, stream_);
  }
  if (has) TE_HIP_CHECK(hipMemcpyAsync(d_mask_.get(), has, (size_t)n_, hipMemcpyHostToDevice, stream_));
  if (pol) {
    // the whole batch in slot order under the policy: the dense gated kernel and, with runs, reacquire_kernel (one tick of
    // step_sequence with the policy as its stream), the NIS row and the event row by slot = by entry in the batch's own rows
    pol_reserve(n_);
    InnovStream is;
    is.nis = pol_nis_dev(); is.ld = n_; is.gate = pol_.nis_max;
    if (pol_.max_rejects >= 0) { is.reacq.on = true; is.reacq.k = pol_.max_rejects; is.reacq.event = pol_event_dev(); is.reacq.ld = n_; }
    else std::fill(pol_event_host(), pol_event_host() + n_, (unsigned char)0);
    step_sequence(1, dt, d_meas_.get(), 0, n_, has ? d_mask_.get() : nullptr, 0, 0, 0, PoseStream{}, is);
  } else {
    step_dense(dt, meas_aos ? d_meas_.get() : nullptr, n_, (meas_aos && has) ? d_mask_.get() : nullptr);
  }
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipStreamSynchronize(stream_));  // caller's host arrays may be reused after return
  if (pol) {
    if (nis_out) std::copy(pol_nis_host(), pol_nis_host() + n_, nis_out);
    if (event_out) std::copy(pol_event_host(), pol_event_host() + n_, event_out);
  }
}

void Batch::step_dense_host_soa(double dt, const void* meas_soa, long ld_host, const unsigned char* has) {
  touch();
  if (n_ == 0) return;
  if (meas_soa && ld_host < n_) throw std::invalid_argument("target_estimation_amd: step_host: the row stride of the host measurements is smaller than the batch");
  stage_reserve(n_);
  if (meas_soa) {
    const bool angular = (type_ == ANGULAR_RATES || type_ == ANGULAR_VELOCITIES);
    const size_t es = elem_size();
    // rows of the device staging block are stage_cap_ elements apart
    TE_HIP_CHECK(hipMemcpy2DAsync(d_meas_.get(), (size_t)stage_cap_ * es, meas_soa, (size_t)ld_host * es, (size_t)n_ * es,
                                  angular ? 7 : 3, hipMemcpyHostToDevice, stream_));
  }
  if (has) TE_HIP_CHECK(hipMemcpyAsync(d_mask_.get(), has, (size_t)n_, hipMemcpyHostToDevice, stream_));
  host_meas_rows_ = (type_ == ANGULAR_RATES || type_ == ANGULAR_VELOCITIES) ? 7 : 3;   // what was transported (measured_pose.hpp)
  step_dense(dt, meas_soa ? d_meas_.get() : nullptr, stage_cap_, (meas_soa && has) ? d_mask_.get() : nullptr);
  host_meas_rows_ = 7;
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipStreamSynchronize(stream_));  // caller's host arrays may be reused after return
}

void Batch::step_one(long slot, double dt, const double* meas7, long out_pos) {
  if (pending_mark_.size() < (size_t)n_) pending_mark_.resize((size_t)n_, 0);
  if (pending_mark_[(size_t)slot]) flush();   // second step of the same target: keep the caller's order
  Pending p;
  p.slot = (int)slot; p.has = meas7 ? 1 : 0; p.dt = dt; p.out = out_pos;
  for (int c = 0; c < 7; ++c) p.meas[c] = meas7 ? meas7[c] : 0.0;
  pending_.push_back(p);
  pending_mark_[(size_t)slot] = 1;
}

void Batch::pin_reserve(long k) {
  if (k <= pin_cap_) return;
  const long want = (std::max<long>(std::max<long>(k, 64), pin_cap_ * 2) + 15) / 16 * 16;   // keeps the sections aligned
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  pin_cap_ = 0; d_pin_ = nullptr;
  h_pin_.alloc((size_t)want * (sizeof(int) + sizeof(double) + 7 * elem_size() + 1) + 64, kPinnedMapped);
  d_pin_ = h_pin_.dev();
  pin_cap_ = want;
}

void Batch::cache_reserve(long n) {
  if (n <= cache_cap_) return;
  const long want = std::max<long>(std::max<long>(n, 64), std::min<long>(cache_cap_ * 2, n > kCacheMax ? kCacheBigMax : kCacheMax));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  cache_cap_ = 0; d_cache_ = nullptr;
  h_cache_.alloc(19 * (size_t)want, kPinnedMapped);
  d_cache_ = h_cache_.dev();
  cache_cap_ = want;
  cache_valid_ = false;
}

// TE_SPIN_WAIT=0 keeps the stream synchronisation (e.g. to leave the core to other threads)
static bool spin_wait_enabled() {
  static const bool on = [] { const char* e = std::getenv("TE_SPIN_WAIT"); return !(e && e[0] == '0'); }();
  return on;
}

void Batch::flush() {
  if (live_.zombie) {              // a resident kernel that never started in time: told to stop, it leaves the records as they are
    live_.zombie = false;
    const hipError_t e = hipStreamSynchronize(live_.stream.get());
    live_release();
    TE_HIP_CHECK(e);
  }
  if (live_.active) live_stop();   // the records in HBM are stale while a live kernel holds the state
  flush_inits();                   // queued creations first: a queued step may be for one of them
  const long k = (long)pending_.size();
  if (!k) return;
  nm_valid_ = false; nm_reads_ = 0;   // the stepped targets' counters change
  // The queue is written by the host and read by the kernel.  A flush of up to one wavefront of targets -- the latency path: the
  // reference's own loop steps one target and reads it back -- goes through a small block in fine-grained DEVICE memory that the host
  // writes through the PCIe BAR (large-BAR systems): posted writes, and the kernel's reads are local instead of four PCIe read round
  // trips at its head (the reference's loop 10.3 -> 8.5 us per cycle for uniform_velocity, 14.3 -> 12.3 for the EKF,
  // profiles/r04_bar_queue.txt; 90 tests and the one-target fuzz run through it: the block is reused by every flush and never read
  // stale).  Larger flushes keep the host-mapped block: the kernel's bulk reads pipeline over PCIe and cached host stores are
  // faster than write-combined ones (400 targets: 41 against 45 us).  TE_QUEUE_BAR=0: always host-mapped.
  constexpr long kBarQueue = 64;
  static const bool bar_wanted = [] { const char* e = std::getenv("TE_QUEUE_BAR"); return !(e && e[0] == '0'); }();
  const size_t es = elem_size();
  if (bar_wanted && !bar_pin_ && !bar_pin_failed_ && k <= kBarQueue) {
    int dev = 0, large_bar = 0;
    if (!(hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) == hipSuccess && large_bar &&
          bar_pin_.try_alloc_finegrained((size_t)kBarQueue * (sizeof(int) + sizeof(double) + 7 * sizeof(double) + 1) + 64))) {
      (void)hipGetLastError();
      bar_pin_failed_ = true;
    }
  }
  const bool use_bar = bar_wanted && bar_pin_ && k <= kBarQueue;
  if (!use_bar) pin_reserve(k);
  char* const hq = use_bar ? bar_pin_.get() : h_pin_.host();   // as the host writes it (never reads it: the BAR mapping is write-combined)
  char* const dq = use_bar ? bar_pin_.get() : d_pin_;   // as the kernel reads it
  const long qcap = use_bar ? kBarQueue : pin_cap_;
  // sections of the block (sized by its capacity, so that the offsets are 8-byte aligned)
  const size_t off_dt = (size_t)qcap * sizeof(int), off_meas = off_dt + (size_t)qcap * sizeof(double),
               off_has = off_meas + (size_t)qcap * 7 * es;
  int* h_idx = reinterpret_cast<int*>(hq);
  double* h_dt = reinterpret_cast<double*>(hq + off_dt);
  unsigned char* h_has = reinterpret_cast<unsigned char*>(hq + off_has);
  bool all_has = true, any_has = false;
  std::vector<long> outs;   // the entries' positions in the gate sink
  if (sink_nis_ || sink_event_) {
    outs.resize((size_t)k);
    for (long j = 0; j < k; ++j) outs[(size_t)j] = pending_[(size_t)j].out;
  }
  for (long j = 0; j < k; ++j) {
    const Pending& p = pending_[(size_t)j];
    h_idx[j] = p.slot; h_dt[j] = p.dt; h_has[j] = p.has;
    // SoA [7][k] in the batch precision (what pack_meas produces on the device)
    if (dtype_ == F64) { double* m = reinterpret_cast<double*>(hq + off_meas); for (int c = 0; c < 7; ++c) m[(size_t)c * k + j] = p.meas[c]; }
    else { float* m = reinterpret_cast<float*>(hq + off_meas); for (int c = 0; c < 7; ++c) m[(size_t)c * k + j] = (float)p.meas[c]; }
    all_has = all_has && p.has;
    any_has = any_has || p.has;
    pending_mark_[(size_t)p.slot] = 0;
  }
  pending_.clear();
  if (use_bar) __builtin_ia32_sfence();   // write-combined on the host: out before the launch
  StepParams p = base_params();
  p.n = k; p.idx = reinterpret_cast<const int*>(dq);
  p.meas = any_has ? dq + off_meas : nullptr; p.meas_ld = k;
  p.has_meas = (any_has && !all_has) ? reinterpret_cast<const unsigned char*>(dq + off_has) : nullptr;
  p.dt_per = reinterpret_cast<const double*>(dq + off_dt); p.dt = 0.0;
  // the update policy: the gated indexed kernel in place of the plain one, still one launch (each entry gated with its own dt);
  // its NIS row and event row are host-mapped rows of their own, not part of the (possibly write-combined) queue block
  const bool pol = pol_.on() && any_has;
  if (pol) fill_update_gate(p, k);
  // With a current getter table the flush reports its own completion through a flag in host-mapped memory and the host
  // spins on it instead of synchronising the stream (tools/launch_latency.hip: the runtime's completion path costs 4 us more
  // than a PCIe write).  Up to one wavefront of queued targets the step kernel itself writes the table rows and the flag --
  // ONE launch per flush; up to one workgroup of the outputs kernel that kernel does.
  // Round 4: beyond one wavefront of targets (up to kFusedFlushMax) the step kernel still does it all -- its wavefronts count
  // themselves in and the last one writes the flag (signal_done) -- instead of a second launch and, beyond one workgroup of
  // the outputs kernel, the runtime's wait (from C, 65 targets: 16.4 -> 12.x us per update + read-back tick; TE_FUSED_FLUSH_MAX).
  static const long fused_max = [] { const char* e = std::getenv("TE_FUSED_FLUSH_MAX"); return e && *e ? std::atol(e) : kFusedFlushMax; }();
  int seq = 0;
  if (cache_valid_ && spin_wait_enabled() && k <= std::max<long>(std::max<long>(ops_->L.tpw, kOutputsBlock), fused_max)) {
    if (!h_done_) {
      PinnedBuf<int> done;
      done.alloc(64 / sizeof(int), kPinnedMapped);
      *done.host() = 0;
      d_done_count_.alloc(64 / sizeof(int));   // the wavefront counter of multi-wavefront flushes: zero between launches
      TE_HIP_CHECK(hipMemsetAsync(d_done_count_.get(), 0, 64, stream_));
      h_done_ = std::move(done); d_done_ = h_done_.dev();   // (last: the flag's presence stands for the counter's too)
    }
    seq = (int)(++done_seq_ & 0x7fffffffu);   // never 0 (= "no flag"), wraps without overflow
    if (seq == 0) seq = (int)(++done_seq_ & 0x7fffffffu);
  }
  const bool fused = seq != 0 && k <= std::max<long>(ops_->L.tpw, fused_max);
  if (fused) {
    p.o_pose = d_cache_; p.o_twist = d_cache_ + 7 * n_; p.o_acc = d_cache_ + 13 * n_;
    p.done_flag = d_done_; p.done_seq = seq; p.done_count = d_done_count_.get();
  }
  launch_step(p, stream_);
  if (cache_valid_ && !fused) {   // keep the getter table current: only the stepped slots change
    OutArgs a;
    a.rec = records_as_stored(); a.idx = p.idx; a.n = k; a.by_slot = 1;
    a.pose = d_cache_; a.twist = d_cache_ + 7 * n_; a.acc = d_cache_ + 13 * n_;
    a.at_time = 0; a.t1 = 0.0; a.t_acc = t_acc_; a.t_base = d_tbase_.get();
    if (seq != 0 && k <= kOutputsBlock) { a.done_flag = d_done_; a.done_seq = seq; }
    else seq = 0;
    ops_->outputs(a, stream_);
  }
  TE_HIP_CHECK(hipGetLastError());
  // the pinned block is rewritten by the next flush, and the getters read the table right after this call
  if (seq != 0) wait_done(seq);
  else TE_HIP_CHECK(hipStreamSynchronize(stream_));
  for (size_t j = 0; j < outs.size(); ++j) {
    if (outs[j] < 0) continue;
    if (sink_nis_) sink_nis_[outs[j]] = pol ? pol_nis_host()[j] : -1.0;
    if (sink_event_) sink_event_[outs[j]] = pol ? pol_event_host()[j] : (unsigned char)0;
  }
}

void Batch::wait_done(int seq) {
  // The signalling kernel is the last launch of the flush (in-order stream): once its flag is here, the step kernel has
  // consumed the pinned inputs and the table rows are in host memory.  A round trip takes 10-20 us; after 2 ms of spinning
  // something else is going on (a busy device, a debugger) and the runtime's own wait takes over.
  const volatile int* flag = h_done_.host();
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return;
    __builtin_ia32_pause();
    if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
  }
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::outputs(const int* slots, long n, double* pose, double* twist, double* acc, bool at_time, double t1) {
  flush();
  if (n <= 0) return;
  stage_reserve(n);
  if (slots) upload_slots(slots, n);
  OutArgs a;
  a.rec = records_as_stored(); a.idx = slots ? d_idx_.get() : nullptr; a.n = n;
  a.pose = pose ? d_aos_.get() : nullptr; a.twist = twist ? d_aos_.get() + 7 * n : nullptr; a.acc = acc ? d_aos_.get() + 13 * n : nullptr;
  a.at_time = at_time ? 1 : 0; a.t1 = t1; a.t_acc = t_acc_; a.t_base = d_tbase_.get();
  ops_->outputs(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
  if (pose) TE_HIP_CHECK(hipMemcpyAsync(pose, a.pose, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, stream_));
  if (twist) TE_HIP_CHECK(hipMemcpyAsync(twist, a.twist, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, stream_));
  if (acc) TE_HIP_CHECK(hipMemcpyAsync(acc, a.acc, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::outputs_dev(double* pose_dev, double* twist_dev, double* acc_dev, bool at_time, double t1) {
  flush();
  if (n_ == 0) return;
  OutArgs a;
  a.rec = records_as_stored(); a.idx = nullptr; a.n = n_; a.pose = pose_dev; a.twist = twist_dev; a.acc = acc_dev;
  a.at_time = at_time ? 1 : 0; a.t1 = t1; a.t_acc = t_acc_; a.t_base = d_tbase_.get();
  ops_->outputs(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::outputs_rows_dev(double* pose_dev, const int* row_of_slot_dev) {
  flush();
  if (n_ == 0) return;
  OutArgs a;
  a.rec = records_as_stored(); a.idx = nullptr; a.n = n_; a.pose = pose_dev; a.twist = nullptr; a.acc = nullptr;
  a.at_time = 0; a.t1 = 0.0; a.t_acc = t_acc_; a.t_base = d_tbase_.get(); a.row_of_slot = row_of_slot_dev;
  ops_->outputs_rows(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::outputs_one(long slot, double* pose, double* twist, double* acc, bool at_time, double t1) {
  flush();
  const int one = (int)slot;
  ++epoch_getters_;
  const bool big = n_ > kCacheMax;
  if (at_time || n_ > kCacheBigMax || (big && !cache_valid_ && !big_sweeps_ && epoch_getters_ <= kBigDirect)) {
    outputs(&one, 1, pose, twist, acc, at_time, t1);
    return;
  }
  // a host-resident table of every slot's outputs, written by the kernels themselves; filled once, then kept current by
  // flush().  Small batches (the reference's scale) always; large ones when the caller sweeps them (batch_store.hpp)
  if (!cache_valid_) {
    cache_reserve(n_);
    OutArgs a;
    a.rec = records_as_stored(); a.idx = nullptr; a.n = n_;
    a.pose = d_cache_; a.twist = d_cache_ + 7 * n_; a.acc = d_cache_ + 13 * n_;
    a.at_time = 0; a.t1 = 0.0; a.t_acc = t_acc_; a.t_base = d_tbase_.get();
    ops_->outputs(a, stream_);
    TE_HIP_CHECK(hipGetLastError());
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    cache_valid_ = true;
  }
  if (pose) std::memcpy(pose, h_cache_.host() + (size_t)slot * 7, sizeof(double) * 7);
  if (twist) std::memcpy(twist, h_cache_.host() + (size_t)n_ * 7 + (size_t)slot * 6, sizeof(double) * 6);
  if (acc) std::memcpy(acc, h_cache_.host() + (size_t)n_ * 13 + (size_t)slot * 6, sizeof(double) * 6);
}

void Batch::intersect(const int* slots, long n, double t1, const double* origin, double radius, double* delta, double* pose) {
  flush();
  if (n <= 0) return;
  stage_reserve(n);
  if (slots) upload_slots(slots, n);
  IntersectArgs a;
  a.rec = records_as_stored(); a.idx = slots ? d_idx_.get() : nullptr; a.n = n; a.t1 = t1;
  a.origin[0] = origin[0]; a.origin[1] = origin[1]; a.origin[2] = origin[2]; a.radius = radius;
  a.t_acc = t_acc_; a.t_base = d_tbase_.get();
  a.delta = d_aos_.get(); a.pose = pose ? d_aos_.get() + n : nullptr;
  ops_->intersect(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipMemcpyAsync(delta, a.delta, sizeof(double) * n, hipMemcpyDeviceToHost, stream_));
  if (pose) TE_HIP_CHECK(hipMemcpyAsync(pose, a.pose, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::intersect_dev(double t1, const double* origin, double radius, double* delta_dev, double* pose_dev) {
  flush();
  if (n_ == 0) return;
  IntersectArgs a;
  a.rec = records_as_stored(); a.idx = nullptr; a.n = n_; a.t1 = t1;
  a.origin[0] = origin[0]; a.origin[1] = origin[1]; a.origin[2] = origin[2]; a.radius = radius;
  a.t_acc = t_acc_; a.t_base = d_tbase_.get(); a.delta = delta_dev; a.pose = pose_dev;
  ops_->intersect(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::gate_reset(long first, long count) {
  if (count <= 0 || !d_gate_ring_) return;
  const int W = gate_window_;
  TE_HIP_CHECK(hipMemsetAsync(d_gate_ring_.get() + first * 2 * W, 0, sizeof(double) * 2 * W * count, stream_));
  TE_HIP_CHECK(hipMemsetAsync(d_gate_sum_.get() + first * 2, 0, sizeof(double) * 2 * count, stream_));
  TE_HIP_CHECK(hipMemsetAsync(d_gate_state_.get() + first * 2, 0, sizeof(int) * 2 * count, stream_));
  hipLaunchKernelGGL(gate_reset_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream_, d_gate_prev_.get(), first, count);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::gate_reserve(int window) {
  if (window <= 0 || window >= (1 << 30)) throw std::runtime_error("target_estimation_amd: bad filters_length");
  if (window == gate_window_ && gate_cap_ >= cap_) return;
  const bool keep = (window == gate_window_) && d_gate_ring_;
  const long old_cap = gate_cap_;
  DeviceBuf<double> ring, sum, prev;
  DeviceBuf<int> st;
  ring.alloc((size_t)2 * window * cap_);
  sum.alloc((size_t)2 * cap_);
  st.alloc((size_t)2 * cap_);
  prev.alloc((size_t)7 * cap_);
  if (keep) {
    TE_HIP_CHECK(hipMemcpyAsync(ring.get(), d_gate_ring_.get(), sizeof(double) * 2 * window * old_cap, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(sum.get(), d_gate_sum_.get(), sizeof(double) * 2 * old_cap, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(st.get(), d_gate_state_.get(), sizeof(int) * 2 * old_cap, hipMemcpyDeviceToDevice, stream_));
    TE_HIP_CHECK(hipMemcpyAsync(prev.get(), d_gate_prev_.get(), sizeof(double) * 7 * old_cap, hipMemcpyDeviceToDevice, stream_));
  }
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  d_gate_ring_ = std::move(ring); d_gate_sum_ = std::move(sum); d_gate_state_ = std::move(st); d_gate_prev_ = std::move(prev);
  gate_window_ = window;
  gate_cap_ = cap_;
  gate_reset(keep ? old_cap : 0, keep ? cap_ - old_cap : cap_);
}

void Batch::gate_move(long src, long dst) {
  if (!d_gate_ring_ || src >= gate_cap_ || dst >= gate_cap_) return;
  const int W = gate_window_;
  TE_HIP_CHECK(hipMemcpyAsync(d_gate_ring_.get() + dst * 2 * W, d_gate_ring_.get() + src * 2 * W, sizeof(double) * 2 * W, hipMemcpyDeviceToDevice, stream_));
  TE_HIP_CHECK(hipMemcpyAsync(d_gate_sum_.get() + dst * 2, d_gate_sum_.get() + src * 2, sizeof(double) * 2, hipMemcpyDeviceToDevice, stream_));
  TE_HIP_CHECK(hipMemcpyAsync(d_gate_state_.get() + dst * 2, d_gate_state_.get() + src * 2, sizeof(int) * 2, hipMemcpyDeviceToDevice, stream_));
  TE_HIP_CHECK(hipMemcpyAsync(d_gate_prev_.get() + dst * 7, d_gate_prev_.get() + src * 7, sizeof(double) * 7, hipMemcpyDeviceToDevice, stream_));
}

void Batch::intersect_gated(const int* slots, long n, double t1, const double* origin, double radius, double pos_th,
                            double ang_th, int window, double* delta, double* pose, unsigned char* converged, double* filt) {
  flush();
  if (n <= 0) return;
  gate_reserve(window);
  stage_reserve(n);
  if (slots) upload_slots(slots, n);
  IntersectArgs a;
  a.rec = records_as_stored(); a.idx = slots ? d_idx_.get() : nullptr; a.n = n; a.t1 = t1;
  a.origin[0] = origin[0]; a.origin[1] = origin[1]; a.origin[2] = origin[2]; a.radius = radius;
  a.t_acc = t_acc_; a.t_base = d_tbase_.get();
  a.delta = d_aos_.get(); a.pose = d_aos_.get() + n;                 // [n] + [n][7]
  ops_->intersect(a, stream_);
  GateArgs g;
  g.idx = a.idx; g.n = n; g.window = gate_window_; g.delta = a.delta; g.pose = a.pose; g.pos_th = pos_th; g.ang_th = ang_th;
  g.ring = d_gate_ring_.get(); g.sum = d_gate_sum_.get(); g.state = d_gate_state_.get(); g.prev = d_gate_prev_.get();
  g.converged = d_mask_.get(); g.filt = filt ? d_aos_.get() + 8 * n : nullptr;   // [n][2] after delta + pose
  g.var = nullptr;
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, stream_, g);
  TE_HIP_CHECK(hipGetLastError());
  if (delta) TE_HIP_CHECK(hipMemcpyAsync(delta, a.delta, sizeof(double) * n, hipMemcpyDeviceToHost, stream_));
  if (pose) TE_HIP_CHECK(hipMemcpyAsync(pose, a.pose, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, stream_));
  if (converged) TE_HIP_CHECK(hipMemcpyAsync(converged, d_mask_.get(), (size_t)n, hipMemcpyDeviceToHost, stream_));
  if (filt) TE_HIP_CHECK(hipMemcpyAsync(filt, g.filt, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::intersect_gated_dev(double t1, const double* origin, double radius, double pos_th, double ang_th, int window,
                                double* delta_dev, double* pose_dev, unsigned char* converged_dev) {
  if (n_ == 0) return;
  intersect_dev(t1, origin, radius, delta_dev, pose_dev);
  gate_update_dev(delta_dev, pose_dev, pos_th, ang_th, window, converged_dev, nullptr, nullptr);
}

void Batch::gate_update_dev(const double* delta_dev, const double* pose_dev, double pos_th, double ang_th, int window,
                            unsigned char* converged_dev, double* filt_dev, double* var_dev) {
  flush();
  if (n_ == 0) return;
  gate_reserve(window);
  GateArgs g;
  g.idx = nullptr; g.n = n_; g.window = gate_window_; g.delta = delta_dev; g.pose = pose_dev; g.pos_th = pos_th; g.ang_th = ang_th;
  g.ring = d_gate_ring_.get(); g.sum = d_gate_sum_.get(); g.state = d_gate_state_.get(); g.prev = d_gate_prev_.get();
  g.converged = converged_dev; g.filt = filt_dev; g.var = var_dev;
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((n_ + 127) / 128)), dim3(128), 0, stream_, g);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::pack_meas_dev(const double* aos_dev, long n, void* soa_dev, long ld) {
  ops_->pack_meas(aos_dev, n, soa_dev, ld, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::get_state(const int* slots, long n, double* x, double* P) {
  flush();
  if (n <= 0) return;
  const int N = ops_->L.n;
  stage_reserve(n);
  if (slots) upload_slots(slots, n);
  // scratch: up to kStateScratchKeep bytes are kept between calls (a caller reading one target's covariance at a time -- the
  // reference test's getEstimator()->getP() -- pays no allocation, and no free: that synchronises the whole device, a
  // resident kernel of another batch included); larger requests are freed again
  const size_t bx = x ? sizeof(double) * (size_t)N * n : 0, bP = P ? sizeof(double) * (size_t)N * N * n : 0;
  DeviceBuf<char> big;
  char* buf = nullptr;
  if (bx + bP <= kStateScratchKeep) {
    if (bx + bP > state_scratch_bytes_) {
      TE_HIP_CHECK(hipStreamSynchronize(stream_));
      state_scratch_bytes_ = 0;
      const size_t want = std::max<size_t>(bx + bP, std::min<size_t>(2 * state_scratch_bytes_ + 4096, kStateScratchKeep));
      d_state_scratch_.alloc(want);
      state_scratch_bytes_ = want;
    }
    buf = d_state_scratch_.get();
  } else {
    big.alloc(bx + bP);
    buf = big.get();
  }
  double* dx = x ? reinterpret_cast<double*>(buf) : nullptr;
  double* dP = P ? reinterpret_cast<double*>(buf + bx) : nullptr;
  ops_->get_state(records_as_stored(), slots ? d_idx_.get() : nullptr, n, dx, dP, ut_flagged_ ? d_tile_blk_.get() : nullptr, ut_flagged_ ? d_tile_uni_.get() : nullptr, stream_);
  TE_HIP_CHECK(hipGetLastError());
  if (x) TE_HIP_CHECK(hipMemcpyAsync(x, dx, bx, hipMemcpyDeviceToHost, stream_));
  if (P) TE_HIP_CHECK(hipMemcpyAsync(P, dP, bP, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Batch::set_state(const int* slots, long n, const double* x, const double* P, const double* unwrap) {
  touch();
  demote_shared();   // a caller's P need not have equal blocks on the axes of a kind
  if (n <= 0) return;
  const int N = ops_->L.n;
  stage_reserve(n);
  if (slots) upload_slots(slots, n);
  DeviceBuf<double> dx, dP, du;
  if (x) { dx.alloc((size_t)N * n); TE_HIP_CHECK(hipMemcpyAsync(dx.get(), x, sizeof(double) * N * n, hipMemcpyHostToDevice, stream_)); }
  if (P) { dP.alloc((size_t)N * N * n); TE_HIP_CHECK(hipMemcpyAsync(dP.get(), P, sizeof(double) * N * N * n, hipMemcpyHostToDevice, stream_)); }
  if (unwrap) { du.alloc((size_t)3 * n); TE_HIP_CHECK(hipMemcpyAsync(du.get(), unwrap, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream_)); }
  ops_->set_state(records(), slots ? d_idx_.get() : nullptr, n, dx.get(), dP.get(), du.get(), stream_);
  TE_HIP_CHECK(hipGetLastError());
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
}

long long Batch::n_measurements(long slot) {
  flush();
  // a caller that asks target after target (get_n_measurements is one of the reference's ten symbols) gets a host copy of all
  // the counters after a few single reads; any step drops it (flush() with queued steps, touch())
  if (!nm_valid_ && ++nm_reads_ > kCounterDirect) {
    h_nm_.resize((size_t)n_);
    TE_HIP_CHECK(hipMemcpyAsync(h_nm_.data(), d_nmbase_.get(), sizeof(int) * (size_t)n_, hipMemcpyDeviceToHost, stream_));
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
    nm_valid_ = true;
  }
  if (nm_valid_) return (long long)h_nm_[(size_t)slot] + nm_acc_;
  int v = 0;
  TE_HIP_CHECK(hipMemcpyAsync(&v, d_nmbase_.get() + slot, sizeof(int), hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  return (long long)v + nm_acc_;
}

void Batch::times(double* out) {
  flush();
  if (n_ == 0) return;
  std::vector<TClock> tb((size_t)n_);
  TE_HIP_CHECK(hipMemcpyAsync(tb.data(), d_tbase_.get(), sizeof(TClock) * n_, hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  for (long i = 0; i < n_; ++i) out[i] = te_clock_time(tb[(size_t)i], t_acc_);
}

double Batch::time(long slot) {
  flush();
  TClock v{0.0, 0.0};
  TE_HIP_CHECK(hipMemcpyAsync(&v, d_tbase_.get() + slot, sizeof(TClock), hipMemcpyDeviceToHost, stream_));
  TE_HIP_CHECK(hipStreamSynchronize(stream_));
  return te_clock_time(v, t_acc_);
}

// ---------------------------------------------------------------- the k soonest crossings (select_soonest.hpp)
void Batch::select_soonest_dev(const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev, double lo, double hi, long k,
                               int* slot_out_dev, double* delta_out_dev, double* pose_out_dev, int* count_out_dev) {
  check_soonest_args(k, lo, hi, delta_dev != nullptr, pose_dev != nullptr, pose_out_dev != nullptr,
                     slot_out_dev != nullptr && delta_out_dev != nullptr && count_out_dev != nullptr);
  if (!soonest_) throw std::logic_error("target_estimation_amd: select_soonest: the batch belongs to no shard");
  soonest_->ensure(soonest_max_wgs_);
  const SoonestPart part{delta_dev, ok_dev, pose_dev, n_, 0};
  launch_select_soonest(&part, 1, lo, hi, (int)k, SoonestOut{nullptr, slot_out_dev, delta_out_dev, pose_out_dev, count_out_dev}, *soonest_, stream_);
}

long Batch::select_soonest(const double* delta_dev, const double* pose_dev, const unsigned char* ok_dev, double lo, double hi, long k,
                           bool with_pose, SoonestRow* rows) {
  check_soonest_args(k, lo, hi, delta_dev != nullptr, pose_dev != nullptr, with_pose, rows != nullptr);
  if (!soonest_) throw std::logic_error("target_estimation_amd: select_soonest: the batch belongs to no shard");
  soonest_->ensure(soonest_max_wgs_);
  const SoonestPart part{delta_dev, ok_dev, pose_dev, n_, 0};
  return select_soonest_to_host(&part, 1, lo, hi, (int)k, with_pose, *soonest_, stream_, rows);
}

// ---------------------------------------------------------------- covariance and time spread at a crossing (crossing_cov.hpp)
void Batch::crossing_cov_dev(double t1, const double* origin, double radius, const double* delta_dev, const int* slots_dev, long n,
                             double sigma_r_max, double sigma_t_max, double* cov_dev, double* sigma_dev, unsigned char* ok_dev,
                             const int* batch_dev, int batch_index) {
  check_crossing_cov_args(delta_dev != nullptr, origin != nullptr, radius, cov_dev != nullptr, sigma_dev != nullptr, ok_dev != nullptr,
                          sigma_r_max, sigma_t_max, slots_dev != nullptr, n, n_);
  const CrossingCovLaunch launch = crossing_cov_launcher(type_, dtype_, ops_->L.g, ops_->L.layout, shared_axes());
  if (!launch) throw std::logic_error("target_estimation_amd: crossing_cov: no kernel for this (model, precision, layout)");   // (never a fall-back)
  flush();
  if (n == 0) return;
  CrossingCovArgs a;
  a.rec = records_as_stored(); a.qr = d_qr_.get(); a.cls = n_classes_ > 1 ? d_cls_.get() : nullptr;
  // (the flag array whenever the batch has one, flagged or not: a captured launch reads the flags of the tick it follows)
  a.tile_blk = d_tile_uni_.get() ? d_tile_blk_.get() : nullptr; a.tile_uni = d_tile_uni_.get();
  a.size = n_; a.n = n; a.slots = slots_dev; a.batch = batch_dev; a.batch_index = batch_index; a.delta = delta_dev;
  a.t1 = t1; a.t_acc = t_acc_; a.t_base = d_tbase_.get();
  a.have_origin = origin ? 1 : 0;
  for (int c = 0; c < 3; ++c) a.origin[c] = origin ? origin[c] : 0.0;
  a.sigma_r_max = sigma_r_max; a.sigma_t_max = sigma_t_max;
  a.cov = cov_dev; a.sigma = sigma_dev; a.ok = ok_dev;
  launch(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::crossing_cov(const int* slots, long n, double t1, const double* origin, double radius, const double* delta, double sigma_r_max,
                         double sigma_t_max, double* cov, double* sigma, unsigned char* ok) {
  check_crossing_cov_args(delta != nullptr, origin != nullptr, radius, cov != nullptr, sigma != nullptr, ok != nullptr, sigma_r_max,
                          sigma_t_max, false, 0, 0);
  if (n <= 0) return;
  if (!slots) throw std::invalid_argument("target_estimation_amd: crossing_cov: a slot list is required");
  for (long done = 0; done < n; done += kCrossingCovMaxRows) {   // a list of any length, kCrossingCovMaxRows rows per launch
    const long k = std::min<long>(kCrossingCovMaxRows, n - done);
    flush();
    stage_reserve(k);
    upload_slots(slots + done, k);
    double* d_delta = d_aos_.get();            // [k] | cov [k][6] | sigma [k][2] of the staging's 19 doubles per entry
    double* d_cov = d_aos_.get() + k;
    double* d_sigma = d_aos_.get() + 7 * k;
    TE_HIP_CHECK(hipMemcpyAsync(d_delta, delta + done, sizeof(double) * k, hipMemcpyHostToDevice, stream_));
    crossing_cov_dev(t1, origin, radius, d_delta, d_idx_.get(), k, sigma_r_max, sigma_t_max, d_cov, sigma ? d_sigma : nullptr, ok ? d_mask_.get() : nullptr);
    TE_HIP_CHECK(hipMemcpyAsync(cov + done * 6, d_cov, sizeof(double) * 6 * k, hipMemcpyDeviceToHost, stream_));
    if (sigma) TE_HIP_CHECK(hipMemcpyAsync(sigma + done * 2, d_sigma, sizeof(double) * 2 * k, hipMemcpyDeviceToHost, stream_));
    if (ok) TE_HIP_CHECK(hipMemcpyAsync(ok + done, d_mask_.get(), (size_t)k, hipMemcpyDeviceToHost, stream_));
    TE_HIP_CHECK(hipStreamSynchronize(stream_));
  }
}

// ---------------------------------------------------------------- association of unlabelled detections (associate.hpp)
void Batch::assoc_table_dev(double dt, AssocRow* rows, int batch_index, double* sdiag, bool sigma_in_w) {
  const AssocTableLaunch launch = assoc_table_launcher(type_, dtype_, ops_->L.g, ops_->L.layout, shared_axes());
  if (!launch) throw std::logic_error("target_estimation_amd: associate: no kernel for this (model, precision, layout)");   // (never a fall-back)
  flush();
  if (n_ == 0) return;
  AssocTableArgs a;
  a.rec = records_as_stored(); a.qr = d_qr_.get(); a.cls = n_classes_ > 1 ? d_cls_.get() : nullptr;
  // (the flag array whenever the batch has one, flagged or not: a captured launch reads the flags of the tick it follows)
  a.tile_blk = d_tile_uni_.get() ? d_tile_blk_.get() : nullptr; a.tile_uni = d_tile_uni_.get();
  a.size = n_; a.dt = dt; a.rows = rows; a.batch_index = batch_index; a.sdiag = sdiag; a.sigma_in_w = sigma_in_w;
  launch(a, stream_);
  TE_HIP_CHECK(hipGetLastError());
}

void associate_batches(Batch* const* batches, int n_batches, AssocScratch& scratch, int forced_chunks, double dt, const double* det_dev, long M,
                       double gate, long rounds, const AssocSlotOut* out, int* slot_of_det, int* batch_of_det, double* d2_of_det, int* info,
                       hipStream_t st, double grid_cell, long forced_buckets) {
  long rows = 0;
  for (int b = 0; b < n_batches; ++b) {
    const LayoutInfo L = batches[b]->layout();
    if (!assoc_table_launcher(batches[b]->type(), batches[b]->dtype(), L.g, L.layout, L.shared_axes != 0))
      throw std::logic_error("target_estimation_amd: associate: no kernel for this (model, precision, layout)");
    rows += batches[b]->size();
  }
  if (rows > 0x7fffffffL) throw std::invalid_argument("target_estimation_amd: associate: more than 2^31 - 1 targets on one device");
  const bool grid = grid_cell > 0.0;
  long off = 0;
  if (grid) {   // the grid form (associate_grid.hpp): one pick per row and per detection, the binning's temporaries
    if (rows + M > 0x7fffffffL) throw std::invalid_argument("target_estimation_amd: associate_grid: more than 2^31 - 1 targets and detections");
    const AssocGridBuckets bk = plan_assoc_grid_call(rows, M, forced_buckets);
    scratch.ensure(rows, M, rows, M);
    scratch.ensure_grid(rows, M, bk.total());
    for (int b = 0; b < n_batches; ++b) {
      batches[b]->assoc_table_dev(dt, scratch.table.get() + off, b, scratch.grid_sdiag.get() + off * 3);
      off += batches[b]->size();
    }
    launch_assoc_grid_match(scratch, rows, det_dev, M, gate, grid_cell, (int)rounds, bk, st);
  } else {
    const AssocGrid gr = plan_assoc_grid(rows, M, forced_chunks), gd = plan_assoc_grid(M, rows, forced_chunks);
    scratch.ensure(rows, M, rows * gr.chunks, M * gd.chunks);
    for (int b = 0; b < n_batches; ++b) {
      batches[b]->assoc_table_dev(dt, scratch.table.get() + off, b);
      off += batches[b]->size();
    }
    launch_assoc_match(scratch, rows, det_dev, M, gate, (int)rounds, forced_chunks, st);
  }
  off = 0;
  for (int b = 0; b < n_batches; ++b) {
    launch_assoc_scatter(batches[b]->dtype(), scratch, off, batches[b]->size(), det_dev, out[b], st);
    off += batches[b]->size();
  }
  launch_assoc_dets(scratch, M, slot_of_det, batch_of_det, d2_of_det, info, st);
  if (grid) launch_assoc_grid_info(scratch, info, st);   // info[3]: the wide slots
  TE_HIP_CHECK(hipGetLastError());
}

void Batch::associate_dev(double dt, const double* det_dev, long M, double gate, long rounds, const AssocSlotOut& out, int* slot_of_det_dev,
                          double* d2_of_det_dev, int* info_dev, double grid_cell) {
  check_assoc_args_for(grid_cell, dt, det_dev != nullptr, M, gate, rounds, out.meas != nullptr && out.has_meas != nullptr && info_dev != nullptr, out.ld, n_);
  if (!assoc_) throw std::logic_error("target_estimation_amd: associate: the batch belongs to no shard");
  Batch* self = this;
  associate_batches(&self, 1, *assoc_, assoc_forced_chunks_, dt, det_dev, M, gate, rounds, &out, slot_of_det_dev, nullptr, d2_of_det_dev, info_dev, stream_,
                    grid_cell, assoc_forced_buckets_);
}

long associate_batches_host(Batch* const* batches, int n_batches, AssocScratch& s, int forced_chunks, double dt, const double* det, long M, double gate,
                            long rounds, const AssocSlotOut* out, unsigned* ids_of_det, int* batch_of_det, int* slot_of_det, double* d2_of_det,
                            long* unmatched, long* n_unmatched, int* info, hipStream_t st, double grid_cell, long forced_buckets) {
  s.ensure_host(M);
  if (M > 0) TE_HIP_CHECK(hipMemcpyAsync(s.det_stage.get(), det, sizeof(double) * 7 * (size_t)M, hipMemcpyHostToDevice, st));
  char* d = s.result_dev.get();
  associate_batches(batches, n_batches, s, forced_chunks, dt, s.det_stage.get(), M, gate, rounds, out, (int*)(d + AssocScratch::off_slot(M)),
                    (int*)(d + AssocScratch::off_batch(M)), (double*)(d + AssocScratch::off_d2(M)), (int*)(d + AssocScratch::off_info(M)), st, grid_cell,
                    forced_buckets);
  TE_HIP_CHECK(hipMemcpyAsync(s.result_host.host(), d, AssocScratch::result_bytes(M), hipMemcpyDeviceToHost, st));
  TE_HIP_CHECK(hipStreamSynchronize(st));
  const char* h = s.result_host.host();
  const int* hs = (const int*)(h + AssocScratch::off_slot(M));
  const int* hb = (const int*)(h + AssocScratch::off_batch(M));
  const double* hd = (const double*)(h + AssocScratch::off_d2(M));
  const int* hi = (const int*)(h + AssocScratch::off_info(M));
  long nu = 0;
  for (long j = 0; j < M; ++j) {
    if (slot_of_det) slot_of_det[j] = hs[j];
    if (batch_of_det) batch_of_det[j] = hb[j];
    if (ids_of_det) ids_of_det[j] = hs[j] >= 0 ? batches[hb[j]]->slot_id(hs[j]) : ~0u;
    if (d2_of_det) d2_of_det[j] = hd[j];
    if (hs[j] < 0) { if (unmatched) unmatched[nu] = j; ++nu; }
  }
  if (n_unmatched) *n_unmatched = nu;
  if (info) for (int c = 0; c < 4; ++c) info[c] = hi[c];
  return hi[0];
}

long Batch::associate(double dt, const double* det, long M, double gate, long rounds, const AssocSlotOut& out, unsigned* ids_of_det,
                      int* slot_of_det, double* d2_of_det, long* unmatched, long* n_unmatched, int* info, double grid_cell) {
  // (the host form's device outputs are optional: without them the call only reports the pairing)
  check_assoc_args_for(grid_cell, dt, det != nullptr, M, gate, rounds, true, out.meas ? out.ld : n_, n_);
  if (!assoc_) throw std::logic_error("target_estimation_amd: associate: the batch belongs to no shard");
  Batch* self = this;
  return associate_batches_host(&self, 1, *assoc_, assoc_forced_chunks_, dt, det, M, gate, rounds, &out, ids_of_det, nullptr, slot_of_det, d2_of_det,
                                unmatched, n_unmatched, info, stream_, grid_cell, assoc_forced_buckets_);
}

}  // namespace te

#ifdef TE_TEST_HOOKS  // only in libtarget_estimation_amd_testhooks.so (csrc/Makefile `testhooks`), never in the product library
// Batch::set_state has no entry in the public headers; tests/test_gpu_uniform_tiles.py reaches it through this one (slots = null:
// slots 0 .. n - 1; x [n][N], P [n][N][N], host arrays).  0, or -1 and the message on stderr.
extern "C" int te_test_batch_set_state(void* batch, long n, const double* x, const double* P) {
  try {
    te::Batch* b = static_cast<te::Batch*>(batch);
    std::unique_lock<std::mutex> l;
    if (b->owner_lock()) l = std::unique_lock<std::mutex>(*b->owner_lock());
    b->set_state(nullptr, n, x, P, nullptr);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "te_test_batch_set_state: %s\n", e.what());
    return -1;
  }
}
#endif
