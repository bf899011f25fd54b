// target_manager.cpp -- see target_manager.hpp.  Every public method: lock, route, call the shard (shard.hpp).
#include "target_manager.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "hip_check.hpp"
#include "yaml_mini.hpp"

namespace te {

using std::lock_guard;
using std::mutex;

static constexpr long kSmallBatchQueue = 1024;   // host-array calls of at most this many targets go through the one-target queue (Shard::updateBatch)

TargetManager::TargetManager(int dtype, int lanes_per_target) {
  settings_.dtype = dtype;
  settings_.lanes = lanes_per_target;
  const char* v = std::getenv("TARGET_ESTIMATION_VERBOSE");
  settings_.verbose = v && v[0] && v[0] != '0';
  // TE_SMALL_BATCH_QUEUE=<n>: the largest call that takes the one-target queue (0 switches it off; the comparison in profiles/)
  static const long most = [] { const char* e = std::getenv("TE_SMALL_BATCH_QUEUE"); return e && *e ? std::atol(e) : kSmallBatchQueue; }();
  settings_.small_batch_most = most;
  static const bool pop = [] { const char* e = std::getenv("TE_POPULATION_TICK"); return !(e && e[0] == '0'); }();
  settings_.population_tick = pop;
  static const bool shared = [] { const char* e = std::getenv("TE_SHARED_AXES"); return !(e && e[0] == '0'); }();
  settings_.shared_axes = shared;
  static const bool uniform = [] { const char* e = std::getenv("TE_UNIFORM_TILES"); return !(e && e[0] == '0'); }();
  settings_.uniform_tiles = uniform;
  // TE_SELECT_SOONEST_MAX_WGS=<n>: the cap on the first-stage workgroups of select_soonest (read per manager, so that one process
  // can hold managers with different grids: tests reach the several-rounds paths at a few thousand entries)
  settings_.soonest_max_wgs = soonest_max_wgs_from(std::getenv("TE_SELECT_SOONEST_MAX_WGS"));
  // TE_ASSOC_COL_CHUNKS=<n>: the column chunks of the association scans, so that small calls exercise the merge of the partials
  settings_.assoc_col_chunks = assoc_forced_chunks_from(std::getenv("TE_ASSOC_COL_CHUNKS"));
  // TE_ASSOC_GRID_BUCKETS=<n>: the buckets of the grid form's hash (a power of two from 1 up), so that small calls live in collisions
  settings_.assoc_grid_buckets = assoc_grid_forced_buckets_from(std::getenv("TE_ASSOC_GRID_BUCKETS"));
  const char* ld = std::getenv("TARGET_ESTIMATION_LOG_DIR");
  if (ld && ld[0]) { log_dir_ = ld; settings_.keep_meas = true; }   // batches created later inherit the measured-pose rows
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    throw std::runtime_error("target_estimation_amd: no HIP device available; this library has no CPU path");
  TE_HIP_CHECK(hipGetDevice(&home_dev_));
  shards_.emplace_back(new Shard(settings_, &target_lock_));
  shard_dev_.assign(1, home_dev_);
}

TargetManager::TargetManager(const std::string& file, int dtype, int lanes_per_target)
    : TargetManager(dtype, lanes_per_target) {
  if (!loadYamlFile(file, default_Q_, default_R_, default_P_, default_type_))
    throw "TargetManager default constructor failed!";
  else
    default_values_loaded_ = true;
}

TargetManager::~TargetManager() {
  for (size_t k = 0; k < shards_.size(); ++k) {
    try { DeviceGuard g(guardDev(k)); shards_[k].reset(); } catch (...) { shards_[k].reset(); }
  }
  closeLogFiles();
}

bool TargetManager::selectTargetType(const std::string& type_str, target_t& type) {
  if (type_str == "angular_rates") type = ANGULAR_RATES;
  else if (type_str == "angular_velocities") type = ANGULAR_VELOCITIES;
  else if (type_str == "uniform_acceleration") type = UNIFORM_ACCELERATION;
  else if (type_str == "uniform_velocity") type = UNIFORM_VELOCITY;
  else return false;
  return true;
}

bool TargetManager::loadYamlFile(const std::string& file, std::vector<double>& Q, std::vector<double>& R,
                                 std::vector<double>& P, target_t& type) {
  bool success = true;
  ModelFile mf;
  std::string err;
  if (!load_model_file(file, mf, err)) {
    std::cerr << err << std::endl;
    return false;
  }
  if (!selectTargetType(mf.type, type)) {
    std::cerr << "Can not parse type: " << mf.type << std::endl;
    std::cerr << "Can not load type from file: " << file << std::endl;
    return false;
  }
  const size_t n = (size_t)model_n((int)type), m = (size_t)model_m((int)type);
  const char* names[3] = {"Q", "R", "P"};
  std::vector<double>* dst[3] = {&Q, &R, &P};
  const size_t want[3] = {n * n, m * m, n * n};
  for (int k = 0; k < 3; ++k) {
    auto it = mf.seqs.find(names[k]);
    if (it == mf.seqs.end() || it->second.size() != want[k]) {
      // the reference maps any square list; its models then assert n (uniform_velocity.cpp:34 ...)
      std::cerr << "Can not load matrix " << names[k] << " from file: " << file << std::endl;
      success = false;
      continue;
    }
    // The reference maps the row-major YAML list column-major (target_manager.cpp:25), i.e. it
    // reads the transpose.  Reproduce that exactly (immaterial for the symmetric shipped models).
    const size_t s = (size_t)std::llround(std::sqrt((double)want[k]));
    dst[k]->assign(want[k], 0.0);
    for (size_t r = 0; r < s; ++r)
      for (size_t c = 0; c < s; ++c) (*dst[k])[r * s + c] = it->second[c * s + r];
  }
  return success;
}

namespace {
// channel order of LogFiles::f / log_all_
const char* const kLogChannel[7] = {"time", "meas_pose", "est_pose", "est_twist", "pose", "est_acc", "covariance"};
}  // namespace

void TargetManager::closeLogFiles() {
  for (auto& kv : log_files_)
    for (std::FILE* f : kv.second.f) if (f) std::fclose(f);
  log_files_.clear();
  for (std::FILE*& f : log_all_) { if (f) std::fclose(f); f = nullptr; }
}

void TargetManager::setLogDirectory(const std::string& dir) {
  {
    lock_guard<mutex> lg(target_lock_);
    closeLogFiles();
    log_dir_ = dir;
  }
  if (!dir.empty()) setKeepMeasurement(true);   // the "measurement" channel needs the rows
}

void TargetManager::setLogTargets(const unsigned* ids, long n) {
  lock_guard<mutex> lg(target_lock_);
  closeLogFiles();
  log_ids_.assign(ids, ids + (n > 0 ? n : 0));
  std::sort(log_ids_.begin(), log_ids_.end());
  log_ids_.erase(std::unique(log_ids_.begin(), log_ids_.end()), log_ids_.end());
}

void TargetManager::setSharedAxes(bool on) {
  lock_guard<mutex> lg(target_lock_);
  for (const auto& sh : shards_)
    if (!sh->batches().empty()) throw std::runtime_error("target_estimation_amd: setSharedAxes: set it before the first target is created");
  settings_.shared_axes = on;
}

void TargetManager::setUniformTiles(bool on) {
  lock_guard<mutex> lg(target_lock_);
  for (const auto& sh : shards_)
    if (!sh->batches().empty()) throw std::runtime_error("target_estimation_amd: setUniformTiles: set it before the first target is created");
  settings_.uniform_tiles = on;
}

void TargetManager::setKeepMeasurement(bool on) {
  lock_guard<mutex> lg(target_lock_);
  settings_.keep_meas = on;
  for (size_t k = 0; k < shards_.size(); ++k) { DeviceGuard g(guardDev(k)); shards_[k]->keepMeasurementChanged(); }
}

// rows into this manager's files: per target (one file per channel and id, kept open) or one <channel>_all file per channel with
// the id in front of every row.  Caller holds target_lock_.
void TargetManager::logWrite(const std::vector<LogRow>& rows, bool per_target) {
  if (per_target) {
    for (const LogRow& r : rows) {
      LogFiles& lf = log_files_[r.id];
      for (int ch = 0; ch < 7; ++ch) {
        if (!lf.f[ch]) {
          lf.f[ch] = std::fopen((log_dir_ + "/" + kLogChannel[ch] + "_" + std::to_string(r.id)).c_str(), "a");
          if (!lf.f[ch]) { std::cerr << "Unable to open file : [" << log_dir_ << "/" << kLogChannel[ch] << "_" << r.id << "]" << std::endl; continue; }
        }
        std::fwrite(r.ch[ch].data(), 1, r.ch[ch].size(), lf.f[ch]);   // one buffered write per channel per call ...
      }
    }
    for (auto& kv : log_files_)
      for (std::FILE* f : kv.second.f) if (f) std::fflush(f);   // ... made visible to readers at the end of the call
    return;
  }
  std::string all[7];
  for (const LogRow& r : rows) {
    char buf[24];
    std::snprintf(buf, sizeof buf, "%g ", (double)r.id);
    for (int ch = 0; ch < 7; ++ch) { all[ch] += buf; all[ch] += r.ch[ch]; }
  }
  for (int ch = 0; ch < 7; ++ch) {
    if (!log_all_[ch]) log_all_[ch] = std::fopen((log_dir_ + "/" + kLogChannel[ch] + "_all").c_str(), "a");
    if (!log_all_[ch]) continue;
    std::fwrite(all[ch].data(), 1, all[ch].size(), log_all_[ch]);
    std::fflush(log_all_[ch]);
  }
}

void TargetManager::log() {
  if (log_dir_.empty()) return;
  lock_guard<mutex> lg(target_lock_);
  // what to log: the explicit selection, or everything while the population is small -- decided once, for the whole manager
  std::vector<unsigned> ids = log_ids_;
  const bool per_target = !ids.empty() || (long)count() <= kLogAutoSelect;
  if (ids.empty()) ids = sortedIds();
  // Every shard reads the rows of its selected targets on its device; the manager writes them all.
  std::vector<LogRow> rows;
  std::vector<std::vector<unsigned>> per(several() ? shards_.size() : 0);
  if (several())
    for (unsigned id : ids) {
      const int k = shard_map_.shard_of(id);
      if (k >= 0) per[(size_t)k].push_back(id);
    }
  for (size_t k = 0; k < shards_.size(); ++k) {
    const std::vector<unsigned>& mine = several() ? per[k] : ids;
    if (mine.empty()) continue;
    DeviceGuard g(guardDev(k));
    const size_t first = rows.size();
    shards_[k]->logCollect(mine, rows);
    if (!several()) continue;
    for (size_t i = first; i < rows.size(); ++i) {   // a shard's batch index -> the manager-wide (model, layout) group
      const Batch& b = *shards_[k]->batches()[(size_t)rows[i].batch];
      const auto key = std::make_pair(b.type(), b.lanes_code());
      rows[i].batch = (int)(std::find(batch_keys_.begin(), batch_keys_.end(), key) - batch_keys_.begin());
    }
  }
  // several shards: in the order one shard would write (batches of one (model, layout) are one group, in order of first
  // creation; ids ascending inside)
  if (several())
    std::stable_sort(rows.begin(), rows.end(), [](const LogRow& a, const LogRow& b) { return a.batch != b.batch ? a.batch < b.batch : a.id < b.id; });
  logWrite(rows, per_target);
}

bool TargetManager::getTargetMeasuredPose(unsigned id, double* pose7) {
  return routeId(id, [&](Shard& s) { return s.measuredPose(id, pose7); });
}

bool TargetManager::getTargetPeriodEstimate(unsigned id, double& period) {
  double twist[6];
  if (!getTargetTwist(id, twist)) return false;
  const double omega_norm = std::sqrt(twist[3] * twist[3] + twist[4] * twist[4] + twist[5] * twist[5]);
  period = omega_norm > 0 ? 2 * M_PI / omega_norm : -1.0;   // target_interface.cpp:82-86
  return true;
}

bool TargetManager::getTargetTransform(unsigned id, double* T) {
  double pose[7];
  if (!getTargetPose(id, pose)) return false;
  double R[9];
  host_quat_to_rot(pose + 3, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = R[r * 3 + c];
    T[r * 4 + 3] = pose[r];
  }
  T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
  return true;
}

bool TargetManager::getTargetDims(unsigned id, int& n, int& m) {
  return routeId(id, [&](Shard& s) { return s.dims(id, n, m); });
}

bool TargetManager::getTargetModelMatrices(unsigned id, double* Q, double* R, double* P0) {
  return routeId(id, [&](Shard& s) { return s.modelMatrices(id, Q, R, P0); });
}

std::vector<unsigned> TargetManager::sortedIds() const {
  if (!several()) return shards_[0]->sortedIds();
  std::vector<std::vector<unsigned>> lists;   // each shard's list is ascending: merged, the whole list is
  for (auto& s : shards_) lists.push_back(s->sortedIds());
  return merge_sorted_ids(lists);
}

std::vector<unsigned> TargetManager::getAvailableTargets() {
  lock_guard<mutex> lg(target_lock_);
  return sortedIds();
}

size_t TargetManager::size() {
  lock_guard<mutex> lg(target_lock_);
  return count();
}

bool TargetManager::hasTarget(unsigned id) {
  lock_guard<mutex> lg(target_lock_);
  return several() ? shard_map_.contains(id) : shards_[0]->contains(id);
}

void TargetManager::init(unsigned id, double dt0, double t0, const double* p0, const double* v0, const double* a0) {
  if (default_values_loaded_)
    init(default_type_, id, dt0, t0, default_Q_.data(), default_R_.data(), default_P_.data(), p0, v0, a0);
  else
    throw "TargetManager::init failed, can not find default values to load!";
}

void TargetManager::init(target_t type, unsigned id, double dt0, double t0, const double* Q, const double* R,
                         const double* P0, const double* p0, const double* v0, const double* a0) {
  (void)dt0;  // only shapes the constructor's A, which every step rebuilds (uniform_velocity.cpp:40,67)
  lock_guard<mutex> lg(target_lock_);
  // several shards: an existing id goes to its shard (which says so); a new one to the placement rule's shard
  size_t k = 0;
  if (several()) {
    const int known = shard_map_.shard_of(id);
    k = (size_t)(known >= 0 ? known : shard_map_.place_one((int)type));
  }
  DeviceGuard g(guardDev(k));
  if (!shards_[k]->init((int)type, id, t0, Q, R, P0, p0, v0, a0)) return;
  ranks_dirty_ = true;
  if (several()) { shard_map_.insert(id, (int)k, (int)type); noteBatchKeys(); }
}

void TargetManager::init(const std::string& file, unsigned id, double dt0, double t0, const double* p0,
                         const double* v0, const double* a0) {
  std::vector<double> Q, R, P;
  target_t type = UNIFORM_VELOCITY;
  if (!loadYamlFile(file, Q, R, P, type)) throw "TargetManager::init failed, can not load the model file!";
  init(type, id, dt0, t0, Q.data(), R.data(), P.data(), p0, v0, a0);
}

long TargetManager::initBatch(const unsigned* ids, long n, double dt0, double t0, const double* p0, const double* v0,
                              const double* a0) {
  if (!default_values_loaded_) throw "TargetManager::init failed, can not find default values to load!";
  return initBatch(default_type_, ids, n, dt0, t0, default_Q_.data(), default_R_.data(), default_P_.data(), false, p0, v0, a0);
}

long TargetManager::initBatch(target_t type, const unsigned* ids, long n, double dt0, double t0, const double* Q,
                              const double* R, const double* P0, bool per_target_P0, const double* p0,
                              const double* v0, const double* a0) {
  (void)dt0;
  lock_guard<mutex> lg(target_lock_);
  return createBatch(type, ids, n, t0, Q, R, P0, per_target_P0, p0, v0, a0, 0, nullptr);
}

long TargetManager::initBatchClasses(target_t type, const unsigned* ids, long n, double dt0, double t0, long n_classes,
                                     const double* Q, const double* R, const double* P0, const unsigned* class_of,
                                     const double* p0, const double* v0, const double* a0) {
  (void)dt0;
  lock_guard<mutex> lg(target_lock_);
  if (n <= 0) return 0;
  if (n_classes <= 0) throw std::invalid_argument("target_estimation_amd: initBatchClasses needs at least one class");
  return createBatch(type, ids, n, t0, Q, R, P0, false, p0, v0, a0, n_classes, class_of);
}

// A batched creation (class_of null: one parameter set).  One shard creates the call as it is.  Several: new ids only (in the
// caller's order), cut into one contiguous run per shard by the placement rule, each run created by its shard.
long TargetManager::createBatch(target_t type, const unsigned* ids, long n, double t0, const double* Q, const double* R, const double* P0,
                                bool per_target_P0, const double* p0, const double* v0, const double* a0, long n_classes,
                                const unsigned* class_of) {
  const int N = model_n((int)type);
  Split sp;
  if (several()) {
    if (class_of)
      for (long i = 0; i < n; ++i)
        if (class_of[i] >= (unsigned long)n_classes) throw std::invalid_argument("target_estimation_amd: class index out of range");
    const std::vector<long> keep = newIdsOnly(ids, n, [&](unsigned id) { return shard_map_.contains(id); }, [&](unsigned id) {
      if (settings_.verbose) std::cout << "Target(" << id << ") already exists!" << std::endl;
    });
    if (keep.empty()) return 0;
    const std::vector<long> amount = shard_map_.place_amounts((int)type, (long)keep.size());
    sp.src.resize(shards_.size());
    long at = 0;
    for (size_t k = 0; k < shards_.size(); at += amount[k], ++k) sp.src[k].assign(keep.begin() + at, keep.begin() + at + amount[k]);
  }
  long created = 0;
  forShards(sp, ids, n, [&](Shard& sh, size_t k, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsIn<double> p2(p0, pos, 7), v2(v0, pos, 6), a2(a0, pos, 6), P2(P0, per_target_P0 ? pos : nullptr, (long)N * N);
    RowsIn<unsigned> cls2(class_of, pos, 1);
    created += class_of ? sh.initBatchClasses((int)type, ids2, m, t0, n_classes, Q, R, P0, cls2.get(), p2.get(), v2.get(), a2.get())
                        : sh.initBatch((int)type, ids2, m, t0, Q, R, P2.get(), per_target_P0, p2.get(), v2.get(), a2.get());
    if (several()) for (long j = 0; j < m; ++j) shard_map_.insert(ids2[j], (int)k, (int)type);
  });
  if (created > 0) ranks_dirty_ = true;
  if (several()) noteBatchKeys();
  return created;
}

bool TargetManager::update(unsigned id, double dt, const double* meas) {
  return routeId(id, [&](Shard& s) { return s.update(id, dt, meas); });
}

bool TargetManager::update(unsigned id, double dt) {
  return update(id, dt, nullptr);
}

void TargetManager::update(double dt) {
  lock_guard<mutex> lg(target_lock_);
  for (size_t k = 0; k < shards_.size(); ++k) { DeviceGuard g(guardDev(k)); shards_[k]->updateAll(dt); }
}

bool TargetManager::erase(unsigned id) {
  lock_guard<mutex> lg(target_lock_);
  const size_t k = shardFor(id);   // (an unknown id: shard 0 says so)
  DeviceGuard g(guardDev(k));
  if (!shards_[k]->erase(id)) return false;
  if (several()) shard_map_.erase(id);
  ranks_dirty_ = true;
  closeLogFilesOf(id);
  return true;
}

long TargetManager::eraseBatch(const unsigned* ids, long n) {
  lock_guard<mutex> lg(target_lock_);
  ranks_dirty_ = true;
  Split sp;
  if (several()) {   // an id leaves the map as it is met, so that a repeated one is unknown the second time, as on one shard
    sp.src.resize(shards_.size());
    for (long i = 0; i < n; ++i) {
      const int k = shard_map_.shard_of(ids[i]);
      if (k < 0) {   // unknown, or already taken by an earlier entry of this call
        std::cout << "Target(" << ids[i] << ") does not exist!" << std::endl;
        continue;
      }
      sp.src[(size_t)k].push_back(i);
      shard_map_.erase(ids[i]);
    }
  }
  long erased = 0;
  std::vector<unsigned> gone;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>*) { erased += sh.eraseBatch(ids2, m, gone); });
  if (!log_files_.empty())
    for (unsigned id : gone) closeLogFilesOf(id);   // logged targets that went away close their files
  return erased;
}

bool TargetManager::getTargetPose(unsigned id, double* pose7) { return getOne(id, pose7, nullptr, nullptr, false, 0.0); }
bool TargetManager::getTargetTwist(unsigned id, double* twist6) { return getOne(id, nullptr, twist6, nullptr, false, 0.0); }
bool TargetManager::getTargetAcceleration(unsigned id, double* acc6) { return getOne(id, nullptr, nullptr, acc6, false, 0.0); }
bool TargetManager::getTargetPoseAt(unsigned id, double t1, double* pose7) { return getOne(id, pose7, nullptr, nullptr, true, t1); }
bool TargetManager::getTargetTwistAt(unsigned id, double t1, double* twist6) { return getOne(id, nullptr, twist6, nullptr, true, t1); }
bool TargetManager::getTargetAccelerationAt(unsigned id, double t1, double* a6) { return getOne(id, nullptr, nullptr, a6, true, t1); }

bool TargetManager::getTargetTime(unsigned id, double& t) {
  return routeId(id, [&](Shard& s) { return s.time(id, t); });
}

int TargetManager::getTargetState(unsigned id, double* x, double* P) {
  return routeId(id, [&](Shard& s) { return s.state(id, x, P); });
}

long long TargetManager::getNumberMeasurements(unsigned id) {
  return routeId(id, [&](Shard& s) { return s.numberMeasurements(id); });
}

int TargetManager::getRejectionRun(unsigned id) {
  return routeId(id, [&](Shard& s) { return s.rejectionRun(id); });
}

// Each shard gets its ids in the caller's order (a repeated id stays two steps in a row) and decides the path for its own slice.
long TargetManager::updateBatch(const unsigned* ids, long n, double dt, const double* meas, const unsigned char* has_meas, double* nis_out,
                                unsigned char* event_out) {
  lock_guard<mutex> lg(target_lock_);
  const Split sp = splitIds(ids, n);
  if (settings_.verbose) for (long i : sp.unknown) std::cout << "Target(" << ids[i] << ") does not exist!" << std::endl;
  // the update policy: every touched batch of every shard must serve it before the first one steps
  bool any_gate = false;
  for (const UpdateGate& g : settings_.gate) any_gate = any_gate || g.on();
  if (any_gate && meas)
    forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>*) { sh.checkUpdateGate(ids2, m); });
  for (long i : sp.unknown) {
    if (nis_out) nis_out[i] = -2.0;
    if (event_out) event_out[i] = 0;
  }
  long done = 0;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsIn<double> m2(meas, pos, 7);
    RowsIn<unsigned char> h2(has_meas, pos, 1);
    RowsOut<double> n2(nis_out, pos, 1);
    RowsOut<unsigned char> e2(event_out, pos, 1);
    done += sh.updateBatch(ids2, m, dt, m2.get(), h2.get(), n2.get(), e2.get());
    scatterAll(n2, e2);
  });
  return done;
}

void TargetManager::setUpdateGate(int type, double nis_max, int max_rejects) {
  check_update_gate(nis_max, max_rejects);
  if (type < -1 || type > 3) throw std::invalid_argument("target_estimation_amd: update gate: no such model type " + std::to_string(type));
  lock_guard<mutex> lg(target_lock_);
  for (int t = 0; t < 4; ++t) {
    if (type >= 0 && t != type) continue;
    settings_.gate[t] = UpdateGate{nis_max, max_rejects};
    for (size_t k = 0; k < shards_.size(); ++k) { DeviceGuard g(guardDev(k)); shards_[k]->updateGateChanged(t); }
  }
}

bool TargetManager::getUpdateGate(int type, double& nis_max, int& max_rejects) {
  if (type < 0 || type > 3) return false;
  lock_guard<mutex> lg(target_lock_);
  nis_max = settings_.gate[type].nis_max; max_rejects = settings_.gate[type].max_rejects;
  return true;
}

int TargetManager::updateGateServed(int type) {
  if (type < 0 || type > 3) return -1;
  lock_guard<mutex> lg(target_lock_);
  int r = -1;
  for (size_t k = 0; k < shards_.size(); ++k) {
    const int s = shards_[k]->updateGateServed(type);
    if (s >= 0) r = (r == 0 || s == 0) ? 0 : 1;
  }
  return r;
}

long TargetManager::getPoseBatch(const unsigned* ids, long n, double* pose, double* twist, double* acc,
                                 unsigned char* found, bool at_time, double t1) {
  lock_guard<mutex> lg(target_lock_);
  const Split sp = splitIds(ids, n);
  if (found) for (long i : sp.unknown) found[i] = 0;
  long done = 0;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsOut<double> p2(pose, pos, 7), t2(twist, pos, 6), a2(acc, pos, 6);
    RowsOut<unsigned char> f2(found, pos, 1);
    done += sh.getPoseBatch(ids2, m, p2.get(), t2.get(), a2.get(), f2.get(), at_time, t1);
    scatterAll(f2, p2, t2, a2);
  });
  return done;
}

long TargetManager::getStateBatch(const unsigned* ids, long n, double* x, double* P) {
  lock_guard<mutex> lg(target_lock_);
  if (n <= 0) return 0;
  const Split sp = splitIds(ids, n);
  if (!sp.unknown.empty()) return -1;
  // several shards: one batch as one shard requires it -- every id of one (model, layout), so one state size
  long ns = -1;
  const Batch* first = nullptr;
  for (size_t k = 0; k < sp.src.size(); ++k)
    for (long i : sp.src[k]) {
      const Batch* b = shards_[k]->batchOf(ids[i]);
      if (!first) { first = b; ns = b->n_state(); }
      if (b->type() != first->type() || b->lanes_code() != first->lanes_code()) return -2;
    }
  long rc = ns;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsOut<double> x2(x, pos, ns), P2(P, pos, ns * ns);
    const long r = sh.getStateBatch(ids2, m, x2.get(), P2.get());
    if (r < 0 || !pos) { rc = r; return; }
    scatterAll(x2, P2);
  });
  return rc;
}

double TargetManager::getIntersectionTimeWithSphere(unsigned id, double t1, const double* origin, double radius) {
  return routeId(id, [&](Shard& s) { return s.intersectTime(id, t1, origin, radius); });
}

bool TargetManager::getIntersectionPoseWithSphere(unsigned id, double t1, const double* origin, double radius,
                                                  double* pose7, double* delta) {
  return routeId(id, [&](Shard& s) { return s.intersectPose(id, t1, origin, radius, pose7, delta); });
}

bool TargetManager::getIntersectionPoseWithSphere(unsigned id, double t1, double pos_th, double ang_th,
                                                  const double* origin, double radius, double* pose7) {
  unsigned char conv = 0, found = 0;
  double delta = -1;
  intersectGatedBatch(&id, 1, t1, pos_th, ang_th, origin, radius, &delta, pose7, &conv, &found);
  return conv != 0;
}

long TargetManager::intersectGatedBatch(const unsigned* ids, long n, double t1, double pos_th, double ang_th,
                                        const double* origin, double radius, double* delta, double* pose,
                                        unsigned char* converged, unsigned char* found, double* filt) {
  lock_guard<mutex> lg(target_lock_);
  const Split sp = splitIds(ids, n);
  for (long i : sp.unknown) {   // what a shard reports for an unknown id
    if (found) found[i] = 0;
    no_intersection(i, delta, pose, converged, filt);
  }
  long done = 0;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsOut<double> d2(delta, pos, 1), p2(pose, pos, 7), f2(filt, pos, 2);
    RowsOut<unsigned char> c2(converged, pos, 1), fd2(found, pos, 1);
    done += sh.intersectGatedBatch(ids2, m, t1, pos_th, ang_th, origin, radius, d2.get(), p2.get(), c2.get(), fd2.get(), f2.get());
    scatterAll(fd2, d2, c2, p2, f2);
  });
  return done;
}

long TargetManager::intersectBatch(const unsigned* ids, long n, double t1, const double* origin, double radius,
                                   double* delta, double* pose, unsigned char* found) {
  lock_guard<mutex> lg(target_lock_);
  const Split sp = splitIds(ids, n);
  for (long i : sp.unknown) {
    if (found) found[i] = 0;
    no_intersection(i, delta, pose, nullptr, nullptr);
  }
  long done = 0;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsOut<double> d2(delta, pos, 1), p2(pose, pos, 7);
    RowsOut<unsigned char> fd2(found, pos, 1);
    done += sh.intersectBatch(ids2, m, t1, origin, radius, d2.get(), p2.get(), fd2.get());
    scatterAll(fd2, d2, p2);
  });
  return done;
}

// ---------------------------------------------------------------- one shard only
void TargetManager::requireOneShard(const char* what) const {
  if (several())
    throw std::runtime_error(std::string("target_estimation_amd: ") + what + " is refused on a manager with more than one shard");
}

static const char* const kLiveMode = "resident mode (target_manager_live_*_all)";

Batch* TargetManager::batchOfType(int type) {
  // with several shards a model has one batch per shard, none of which holds all its targets: refused
  requireOneShard("target_manager_get_batch_of_type (use target_manager_get_batch / target_manager_batch_shard)");
  return shards_[0]->batchOfType(type);
}

long TargetManager::posesToDevice(double* out_dev, long capacity, hipStream_t st) {
  return onlyShard("posesToDevice", [&](Shard& s) {
    const long rows = s.rows();
    if (!out_dev) return rows;
    if (capacity < rows) throw std::invalid_argument("target_estimation_amd: posesToDevice: buffer too small");
    if (st != s.stream()) throw std::invalid_argument("target_estimation_amd: posesToDevice runs on the manager's stream");
    s.posesToDevice(out_dev);
    return rows;
  });
}

long TargetManager::posesForGather(long expect_rows, const std::function<double*(long, hipStream_t)>& prepare) {
  return onlyShard("the RCCL gather", [&](Shard& s) {   // count, stream and the outputs launches in ONE critical section
    const long rows = s.rows();
    if (rows != expect_rows) throw std::invalid_argument("target_estimation_amd: gather: counts[rank] differs from the manager's size");
    double* out_dev = prepare(rows, s.stream());
    if (!out_dev && rows > 0) throw std::invalid_argument("target_estimation_amd: gather: no destination for the pose rows");
    s.posesToDevice(out_dev);
    return rows;
  });
}

void TargetManager::setStream(hipStream_t st) {
  onlyShard("target_manager_set_stream (use target_manager_set_shard_stream)", [&](Shard& s) { s.setStream(st); });
}

void TargetManager::liveStartAll(double dt, const Batch::SeqSpec* specs, long n_specs, long first_entry, long max_ticks, double idle_limit_s,
                                 bool query, const double* origin, double radius) {
  onlyShard(kLiveMode, [&](Shard& s) { s.liveStartAll(dt, specs, n_specs, first_entry, max_ticks, idle_limit_s, query, origin, radius); });
}

void TargetManager::livePostAll(long n_ticks, bool one_doorbell_per_tick) {
  onlyShard(kLiveMode, [&](Shard& s) { s.livePostAll(n_ticks, one_doorbell_per_tick); });
}

long TargetManager::liveDoneAll() {
  return onlyShard(kLiveMode, [](Shard& s) { return s.liveDoneAll(); });
}

bool TargetManager::liveWaitAll(long tick, double timeout_s) {
  // the list under the lock, the spinning without it (posts come from other threads)
  const std::vector<Batch*> open = onlyShard(kLiveMode, [](Shard& s) { return s.liveOpenBatches(); });
  DeviceGuard g(guardDev(0));
  for (Batch* b : open)
    if (!b->live_wait(tick, timeout_s)) return false;
  return true;
}

long TargetManager::liveStopAll() {
  return onlyShard(kLiveMode, [](Shard& s) { return s.liveStopAll(); });
}

// ---------------------------------------------------------------- every shard
bool TargetManager::populationTickNow() {
  lock_guard<mutex> lg(target_lock_);
  bool any = false;   // every shard that holds targets ticks them in one launch
  for (const auto& s : shards_) {
    if (s->size() == 0) continue;
    if (!s->populationTick()) return false;
    any = true;
  }
  return any;
}

void TargetManager::stepSequenceAll(long n_ticks, double dt, const Batch::SeqSpec* specs, const PoseStream* poses, long n_specs, bool query,
                                    const double* origin, double radius, int use_graph, const InnovStream* innov, const DtSchedule& sched) {
  if (n_specs < 0) throw std::invalid_argument("target_estimation_amd: stepSequenceAll: negative number of batches");
  std::vector<Batch::SeqSpec> with((size_t)n_specs);
  for (long b = 0; b < n_specs; ++b) {
    with[(size_t)b] = specs[b];
    with[(size_t)b].poses = poses ? poses[b] : PoseStream{};
    with[(size_t)b].innov = innov ? innov[b] : InnovStream{};
  }
  stepSequenceAll(n_ticks, dt, with.data(), n_specs, query, origin, radius, use_graph, sched);
}

void TargetManager::stepSequenceAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, bool query,
                                    const double* origin, double radius, int use_graph, const DtSchedule& sched) {
  lock_guard<mutex> lg(target_lock_);
  if (sched.on() && sched.n != n_ticks) throw std::invalid_argument("target_estimation_amd: the time-step schedule has one entry per tick of the call");
  if (several()) {   // specs shard-major (numBatches order); a shard checks its own slice, so here every check before any shard launches
    if (n_specs != (long)numBatches()) throw std::runtime_error("target_estimation_amd: stepSequenceAll needs one spec per batch");
    long off = 0;
    for (auto& s : shards_)
      for (auto& b : s->batches()) {
        b->check_pose_stream(specs[off].poses);
        b->check_innov_stream(specs[off].innov);
        if (n_ticks > 0 && query && b->size() > 0 && (!origin || !specs[off].delta_dev))
          throw std::runtime_error("target_estimation_amd: stepSequenceAll: query without an origin or a delta output");
        ++off;
      }
  }
  long off = 0;
  for (size_t k = 0; k < shards_.size(); ++k) {
    const long nk = several() ? (long)shards_[k]->batches().size() : n_specs;
    DeviceGuard g(guardDev(k));
    shards_[k]->stepSequenceAll(n_ticks, dt, specs + off, nk, query, origin, radius, use_graph, sched);
    off += nk;
  }
}

void TargetManager::stepFusedAll(long n_ticks, double dt, const Batch::SeqSpec* specs, long n_specs, const DtSchedule& sched) {
  lock_guard<mutex> lg(target_lock_);
  if (n_specs < 0) throw std::invalid_argument("target_estimation_amd: stepFusedAll: negative number of batches");
  if (sched.on() && sched.n != n_ticks) throw std::invalid_argument("target_estimation_amd: the time-step schedule has one entry per tick of the call");
  if (several()) {   // specs shard-major (numBatches order): every shard's refusals before any shard changes anything
    if (n_specs != (long)numBatches()) throw std::runtime_error("target_estimation_amd: stepFusedAll needs one spec per batch");
    long off = 0;
    for (auto& s : shards_)
      for (auto& b : s->batches()) {
        if (specs[off].ring_ticks != 0) throw std::invalid_argument("target_estimation_amd: stepFusedAll: a fused call reads its measurements linearly (ring_ticks must be 0)");
        b->check_fused_call(n_ticks, specs[off], sched, false);
        ++off;
      }
  }
  long off = 0;
  for (size_t k = 0; k < shards_.size(); ++k) {
    const long nk = several() ? (long)shards_[k]->batches().size() : n_specs;
    DeviceGuard g(guardDev(k));
    shards_[k]->stepFusedAll(n_ticks, dt, specs + off, nk, sched);
    off += nk;
  }
}

int TargetManager::fusedAllServed(bool gated, bool scheduled) {
  lock_guard<mutex> lg(target_lock_);
  bool any = false;   // every shard that holds targets replays them in one launch
  for (const auto& s : shards_) {
    if (s->size() == 0) continue;
    if (!s->fusedAllServed(gated, scheduled)) return 0;
    any = true;
  }
  return any ? 1 : 0;
}

long TargetManager::selectSoonest(const SoonestSpec* specs, long n_specs, double lo, double hi, long k, bool with_pose, SoonestRow* rows,
                                  unsigned* ids) {
  lock_guard<mutex> lg(target_lock_);
  check_soonest_args(k, lo, hi, true, with_pose, with_pose, rows != nullptr && ids != nullptr);
  if (n_specs != (long)numBatches() || (n_specs > 0 && !specs)) throw std::invalid_argument("target_estimation_amd: select_soonest: one description per batch is needed");
  long off = 0;
  for (auto& s : shards_) {   // every shard's refusals before any shard enqueues
    const long nk = (long)s->batches().size();
    s->checkSelectSoonest(specs + off, nk, with_pose);
    off += nk;
  }
  off = 0;
  for (size_t s = 0; s < shards_.size(); ++s) {
    const long nk = (long)shards_[s]->batches().size();
    DeviceGuard g(guardDev(s));
    shards_[s]->selectSoonestBegin(specs + off, nk, (int)off, lo, hi, (int)k, with_pose);
    off += nk;
  }
  std::vector<std::vector<SoonestRow>> per(shards_.size());
  for (size_t s = 0; s < shards_.size(); ++s) {
    DeviceGuard g(guardDev(s));
    per[s].resize((size_t)k);
    per[s].resize((size_t)shards_[s]->selectSoonestEnd((int)k, with_pose, per[s].data()));
  }
  const long count = merge_soonest(per, k, rows);
  for (long i = 0; i < k; ++i) ids[i] = i < count ? batch(rows[i].batch)->slot_id(rows[i].slot) : ~0u;
  return count;
}

void TargetManager::selectSoonestDev(const SoonestSpec* specs, long n_specs, double lo, double hi, long k, const SoonestOut& out) {
  lock_guard<mutex> lg(target_lock_);
  if (several())
    throw std::runtime_error("target_estimation_amd: select_soonest_dev: the manager spans " + std::to_string(shards_.size()) +
                             " shards, so there is no single device to leave the result on (use select_soonest, which merges on the host)");
  check_soonest_args(k, lo, hi, true, out.pose != nullptr, out.pose != nullptr,
                     out.batch != nullptr && out.slot != nullptr && out.delta != nullptr && out.count != nullptr);
  if (n_specs != (long)numBatches() || (n_specs > 0 && !specs)) throw std::invalid_argument("target_estimation_amd: select_soonest: one description per batch is needed");
  DeviceGuard g(guardDev(0));
  shards_[0]->selectSoonestDev(specs, n_specs, 0, lo, hi, (int)k, out);
}

void TargetManager::crossingCovDev(double t1, const double* origin, double radius, const int* batch_dev, const int* slots_dev,
                                   const double* delta_dev, long n, double sigma_r_max, double sigma_t_max, double* cov_dev, double* sigma_dev,
                                   unsigned char* ok_dev) {
  lock_guard<mutex> lg(target_lock_);
  check_crossing_cov_one_shard((long)shards_.size());
  DeviceGuard g(guardDev(0));
  shards_[0]->crossingCovDev(t1, origin, radius, batch_dev, slots_dev, delta_dev, n, sigma_r_max, sigma_t_max, cov_dev, sigma_dev, ok_dev);
}

long TargetManager::crossingCovBatch(const unsigned* ids, long n, double t1, const double* origin, double radius, const double* delta,
                                     double sigma_r_max, double sigma_t_max, double* cov, double* sigma, unsigned char* ok) {
  lock_guard<mutex> lg(target_lock_);
  check_crossing_cov_args(delta != nullptr, origin != nullptr, radius, cov != nullptr, sigma != nullptr, ok != nullptr, sigma_r_max,
                          sigma_t_max, false, 0, 0);
  if (n <= 0) return 0;
  if (!ids) throw std::invalid_argument("target_estimation_amd: crossing_cov: ids are required");
  const Split sp = splitIds(ids, n);
  for (long i : sp.unknown) crossing_cov_fill(i, cov, sigma, ok);
  long done = 0;
  forShards(sp, ids, n, [&](Shard& sh, size_t, const unsigned* ids2, long m, const std::vector<long>* pos) {
    RowsIn<double> d2(delta, pos, 1);
    RowsOut<double> c2(cov, pos, 6), s2(sigma, pos, 2);
    RowsOut<unsigned char> o2(ok, pos, 1);
    done += sh.crossingCovBatch(ids2, m, t1, origin, radius, d2.get(), sigma_r_max, sigma_t_max, c2.get(), s2.get(), o2.get());
    scatterAll(c2, s2, o2);
  });
  return done;
}

void TargetManager::associateDev(double dt, const double* det_dev, long M, double gate, long rounds, const AssocSlotOut* out, long n_out,
                                 int* slot_of_det_dev, int* batch_of_det_dev, double* d2_of_det_dev, int* info_dev, double grid_cell) {
  lock_guard<mutex> lg(target_lock_);
  check_assoc_one_shard((long)shards_.size());
  DeviceGuard g(guardDev(0));
  shards_[0]->associateDev(dt, det_dev, M, gate, rounds, out, n_out, slot_of_det_dev, batch_of_det_dev, d2_of_det_dev, info_dev, grid_cell);
}

long TargetManager::associate(double dt, const double* det, long M, double gate, long rounds, const AssocSlotOut* out, long n_out,
                              unsigned* ids_of_det, int* batch_of_det, int* slot_of_det, double* d2_of_det, long* unmatched, long* n_unmatched,
                              int* info, double grid_cell) {
  lock_guard<mutex> lg(target_lock_);
  check_assoc_one_shard((long)shards_.size());
  DeviceGuard g(guardDev(0));
  return shards_[0]->associate(dt, det, M, gate, rounds, out, n_out, ids_of_det, batch_of_det, slot_of_det, d2_of_det, unmatched, n_unmatched, info, grid_cell);
}

void TargetManager::lifecycle(const double* det_dev, const int* slot_of_det_dev, long M, const unsigned char* const* has_dev, long n_masks,
                              const LifecyclePolicy& policy, unsigned* retired_ids_out, long retired_cap, long* info) {
  lock_guard<mutex> lg(target_lock_);
  requireOneShard("target_manager_lifecycle");
  LifecyclePolicy p = policy;
  if (p.births() && p.defaults()) {
    if (!default_values_loaded_ || (int)default_type_ != p.birth_type)
      throw std::invalid_argument("target_estimation_amd: lifecycle: Q, R and P0 may be left out only when birth_type is the manager's default model");
    p.Q = default_Q_.data(); p.R = default_R_.data(); p.P0 = default_P_.data();
  }
  DeviceGuard g(guardDev(0));
  shards_[0]->lifecycle(det_dev, slot_of_det_dev, M, has_dev, n_masks, p, retired_ids_out, retired_cap, info);
  if (info[0] > 0 || info[1] > 0) ranks_dirty_ = true;
  if (!log_files_.empty())
    for (long j = 0; j < info[0]; ++j) closeLogFilesOf(retired_ids_out[j]);   // logged targets that went away close their files
}

void TargetManager::findDuplicatesDev(double dt, double gate, long rounds, double cell, int min_hits, const MergeSlotOut* out, long n_out,
                                      int* info_dev) {
  lock_guard<mutex> lg(target_lock_);
  check_merge_one_shard("find_duplicates", (long)shards_.size());
  DeviceGuard g(guardDev(0));
  shards_[0]->findDuplicatesDev(dt, gate, rounds, cell, min_hits, out, n_out, info_dev);
}

void TargetManager::retireDuplicates(double dt, double gate, long rounds, double cell, int min_hits, unsigned* retired_ids_out,
                                     unsigned* kept_ids_out, long cap, long* info) {
  lock_guard<mutex> lg(target_lock_);
  check_merge_one_shard("retire_duplicates", (long)shards_.size());
  DeviceGuard g(guardDev(0));
  shards_[0]->retireDuplicates(dt, gate, rounds, cell, min_hits, retired_ids_out, kept_ids_out, cap, info);
  if (info[0] > 0) ranks_dirty_ = true;
  if (!log_files_.empty())
    for (long j = 0; j < info[0]; ++j) closeLogFilesOf(retired_ids_out[j]);   // logged targets that went away close their files
}

bool TargetManager::getTrackCounts(unsigned id, int& miss, int& hits) {
  return routeId(id, [&](Shard& s) { return s.trackCounts(id, miss, hits); });
}

void TargetManager::synchronize() {
  lock_guard<mutex> lg(target_lock_);
  for (size_t k = 0; k < shards_.size(); ++k) { DeviceGuard g(guardDev(k)); shards_[k]->synchronize(); }
}

// ---------------------------------------------------------------- several devices
void DeviceGuard::enter() {
  TE_HIP_CHECK(hipGetDevice(&prev));
  if (prev != dev) TE_HIP_CHECK(hipSetDevice(dev));
}

int TargetManager::numBatches() const {
  int n = 0;
  for (const auto& s : shards_) n += (int)s->batches().size();
  return n;
}

Batch* TargetManager::batch(int i) {
  for (auto& s : shards_) {
    if (i < (int)s->batches().size()) return s->batches()[(size_t)i].get();
    i -= (int)s->batches().size();
  }
  return nullptr;
}

int TargetManager::batchShard(int i) const {
  if (i < 0) return -1;
  for (size_t k = 0; k < shards_.size(); ++k) {
    if (i < (int)shards_[k]->batches().size()) return (int)k;
    i -= (int)shards_[k]->batches().size();
  }
  return -1;
}

int TargetManager::shardDevice(int k) const {
  if (k < 0 || k >= numShards()) return -1;
  return shard_dev_[(size_t)k];
}

int TargetManager::shardOf(unsigned id) {
  lock_guard<mutex> lg(target_lock_);
  if (several()) return shard_map_.shard_of(id);
  return shards_[0]->contains(id) ? 0 : -1;
}

void TargetManager::setDevices(const int* devices, int n) {
  lock_guard<mutex> lg(target_lock_);
  if (count() > 0)
    throw std::runtime_error("target_estimation_amd: set_devices: the manager already holds targets (call it before the first init)");
  if (n < 1) throw std::invalid_argument("target_estimation_amd: set_devices: at least one device is needed");
  if (!devices) throw std::invalid_argument("target_estimation_amd: set_devices: NULL device list");
  if (!placed_ && shards_[0]->stream() != nullptr)   // a stream belongs to one device: the shards would silently fall back to their default streams
    throw std::runtime_error("target_estimation_amd: set_devices after set_stream: set each shard's stream with set_shard_stream instead");
  int count = 0;
  TE_HIP_CHECK(hipGetDeviceCount(&count));
  for (int k = 0; k < n; ++k)
    if (devices[k] < 0 || devices[k] >= count)
      throw std::invalid_argument("target_estimation_amd: set_devices: device index " + std::to_string(devices[k]) + " out of range (" +
                                  std::to_string(count) + " devices)");
  const bool as_constructed = n == 1 && devices[0] == home_dev_;   // one shard on the creation device, no DeviceGuard
  if (as_constructed && !placed_) return;
  std::vector<std::unique_ptr<Shard>> fresh;
  for (int k = 0; k < n; ++k) {
    DeviceGuard g(devices[k]);
    fresh.emplace_back(new Shard(settings_, &target_lock_));
  }
  // Peer access between distinct devices, so that one pose_out reaches every shard (getEstAllById).  Not yet run across
  // devices: the machines this was built on have one GPU.
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      if (devices[a] == devices[b]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) != hipSuccess || !can) continue;
      DeviceGuard g(devices[a]);
      const hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) TE_HIP_CHECK(e);
      (void)hipGetLastError();
    }
  for (size_t k = 0; k < shards_.size(); ++k) { DeviceGuard g(guardDev(k)); shards_[k].reset(); }
  shards_ = std::move(fresh);
  shard_dev_.assign(devices, devices + n);
  placed_ = !as_constructed;
  shard_map_.reset(several() ? n : 0);
  batch_keys_.clear();
  ranks_dirty_ = true;
}

void TargetManager::setShardStream(int k, hipStream_t s) {
  if (k < 0 || k >= numShards()) throw std::invalid_argument("target_estimation_amd: set_shard_stream: no shard " + std::to_string(k));
  lock_guard<mutex> lg(target_lock_);
  DeviceGuard g(guardDev((size_t)k));
  shards_[(size_t)k]->setStream(s);
}

Split TargetManager::splitIds(const unsigned* ids, long n) const {
  Split sp;
  if (!several()) return sp;   // (one shard takes the call whole and answers for unknown ids itself: forShards)
  sp.src.resize(shards_.size());
  for (long i = 0; i < n; ++i) {
    const int k = shard_map_.shard_of(ids[i]);
    if (k < 0) sp.unknown.push_back(i);
    else sp.src[(size_t)k].push_back(i);
  }
  return sp;
}

void TargetManager::noteBatchKeys() {
  for (auto& sh : shards_)
    for (auto& b : sh->batches()) {
      const auto key = std::make_pair(b->type(), b->lanes_code());
      if (std::find(batch_keys_.begin(), batch_keys_.end(), key) == batch_keys_.end()) batch_keys_.push_back(key);
    }
}

void TargetManager::closeLogFilesOf(unsigned id) {
  auto lf = log_files_.find(id);   // a logged target that goes away closes its files (a later target of that id appends)
  if (lf == log_files_.end()) return;
  for (std::FILE* f : lf->second.f) if (f) std::fclose(f);
  log_files_.erase(lf);
}

long TargetManager::getEstAllById(double* pose_out, long capacity) {
  lock_guard<mutex> lg(target_lock_);
  const long rows = (long)count();
  if (!pose_out) return rows;
  if (capacity < rows) throw std::invalid_argument("target_estimation_amd: get_est_all_by_id: capacity " + std::to_string(capacity) +
                                                   " is smaller than the " + std::to_string(rows) + " targets");
  if (rows == 0) return 0;
  if (ranks_dirty_) {
    const std::vector<unsigned> all = sortedIds();
    for (size_t k = 0; k < shards_.size(); ++k) { DeviceGuard g(guardDev(k)); shards_[k]->uploadRanks(all); }
    ranks_dirty_ = false;
  }
  for (size_t k = 0; k < shards_.size(); ++k) {   // every shard's launches on its own stream; none waits for another
    DeviceGuard g(guardDev(k));
    shards_[k]->launchRows(pose_out);
  }
  return rows;
}

}  // namespace te
