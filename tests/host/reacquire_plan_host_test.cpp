// Host test (no HIP) of the re-acquisition's host logic: csrc/step_variant.hpp (plan_step with the request field P::reacq: the
// launch behind the step, the refusals) and csrc/reacquire_plan.hpp (the policy's checks; the bookkeeping of the device copies of
// the initial-covariance table and of the slot -> row index through append, single erase and batched erase).
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/reacquire_plan_host_test.cpp && ./a.out
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../target_estimation_amd/csrc/reacquire_plan.hpp"
#include "../../target_estimation_amd/csrc/step_variant.hpp"

using namespace te;

// the members of StepParams that plan_step reads; a set pointer is `true`
struct Gated {   // (the request type of gate_plan_host_test.cpp: no reacq)
  bool idx = false, cls = false, rec_out = false, q_delta = false, pose = false, nis = false;
  bool o_pose = false, o_twist = false, o_acc = false, done_flag = false, done_count = false;
  bool live_posted = false, live_mirror = false, live_progress = false, live_done = false, live_pose = false;
  bool tile_uni = false, tile_blk = false;
  long live_ring = 0;
  int n_ticks = 1;
  long n = 65;
  double gate = 0.0;
  int gate_by_writer = 0;
};
struct Req : Gated {
  bool meas = true;
  int reacq = 0, reacq_k = 0;
  bool reacq_run = false, reacq_p0 = false, reacq_p0_idx = false;
};

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++g_fail;                                            \
      std::printf("FAIL line %d: %s: ", __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
    }                                                      \
  } while (0)

static const StepTraits kSepPacked{true, false, false, true, false, false, 64};
static const StepTraits kSharedUt{true, true, true, false, false, false, 64};
static const StepTraits kDense{false, false, false, false, false, false, 64};

// "gated: innov, (8) + reacquire + pose"
template <class R>
static std::string run(const StepTraits& t, const R& r) {
  try {
    const StepPlan p = plan_step(t, r);
    std::string s = p.gated ? "gated: " : "";
    if (p.innov_writer_first) s += "innov, ";
    s += "(" + std::to_string(p.variant) + ")";
    if (p.reacquire_after_step) s += " + reacquire";
    if (p.pose_writer_after_each_tick) s += " + pose";
    return s;
  } catch (const std::runtime_error&) {
    return "throws";
  }
}
#define PIN(traits, req, want) CHECK(run(traits, req) == (want), "%s, want %s", run(traits, req).c_str(), std::string(want).c_str())

template <class F>
static std::string refused(F&& f) {
  try { f(); } catch (const std::invalid_argument& e) { return e.what(); }
  return "";
}

static void plan_rows() {
  const std::string innov = std::to_string((unsigned)kInnov);
  static_assert(has_reacq_member<Req>::value && !has_reacq_member<Gated>::value, "the member-detection helper");
  Req g;
  g.nis = true; g.gate = 300.0; g.reacq = 1; g.reacq_k = 3; g.reacq_run = g.reacq_p0 = g.reacq_p0_idx = true;
  // behind the gated kernel, and behind the writer + mask + step triple; ahead of the pose writer
  for (const StepTraits* t : {&kSepPacked, &kSharedUt}) PIN(*t, g, "gated: (" + innov + ") + reacquire");
  PIN(kDense, g, "gated: innov, (0) + reacquire");
  { Req r = g; r.pose = true; PIN(kSepPacked, r, "gated: (" + innov + ") + reacquire + pose"); PIN(kDense, r, "gated: innov, (0) + reacquire + pose"); }
  { Req r = g; r.reacq_k = 0; PIN(kSepPacked, r, "gated: (" + innov + ") + reacquire"); }     // K = 0 counts: still a launch
  { Req r = g; r.reacq_k = 127; PIN(kSepPacked, r, "gated: (" + innov + ") + reacquire"); }
  { Req r = g; r.meas = false; PIN(kSepPacked, r, "gated: (" + innov + ")"); PIN(kDense, r, "gated: innov, (0)"); }   // predict-only: nothing
  { Req r = g; r.reacq = 0; PIN(kSepPacked, r, "gated: (" + innov + ")"); }                     // no policy: the gated plan
  // refused: a policy without a gate, K outside 0..127, a missing table, and everything the gate refuses
  for (const StepTraits* t : {&kSepPacked, &kDense}) {
    { Req r = g; r.gate = 0.0; PIN(*t, r, "throws"); }
    { Req r = g; r.gate = 0.0; r.nis = false; PIN(*t, r, "throws"); }
    { Req r = g; r.reacq_k = -1; PIN(*t, r, "throws"); }
    { Req r = g; r.reacq_k = 128; PIN(*t, r, "throws"); }
    { Req r = g; r.reacq_run = false; PIN(*t, r, "throws"); }
    { Req r = g; r.reacq_p0 = false; PIN(*t, r, "throws"); }
    { Req r = g; r.reacq_p0_idx = false; PIN(*t, r, "throws"); }
    { Req r = g; r.nis = false; PIN(*t, r, "throws"); }
    { Req r = g; r.idx = true; PIN(*t, r, "throws"); }
    { Req r = g; r.n_ticks = 3; PIN(*t, r, "throws"); }
    { Req r = g; r.rec_out = true; PIN(*t, r, "throws"); }
  }
  // a request type without the member plans as before
  { Gated o; o.nis = true; o.gate = 300.0; PIN(kSepPacked, o, "gated: (" + innov + ")"); PIN(kDense, o, "gated: innov, (0)"); }
}

static void policy_checks() {
  unsigned char row[8];
  Reacquire q;
  CHECK(refused([&] { check_reacquire(q, 0.0, 100, true, false); }).empty(), "a policy that is off is never refused");
  q.on = true; q.k = 3;
  CHECK(refused([&] { check_reacquire(q, 300.0, 100, false, true); }).empty(), "a good policy without rows");
  CHECK(refused([&] { check_reacquire(q, 0.0, 100, false, true); }).find("gate") != std::string::npos, "no gate");
  for (int k : {-1, 128, 1000}) { Reacquire r = q; r.k = k; CHECK(!refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "K = %d", k); }
  for (int k : {0, 1, 127}) { Reacquire r = q; r.k = k; CHECK(refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "K = %d", k); }
  q.event = row; q.ld = 100; q.tick_stride = 100;
  CHECK(refused([&] { check_reacquire(q, 300.0, 100, false, true); }).empty(), "good rows");
  { Reacquire r = q; r.ld = 99; r.tick_stride = 99; CHECK(!refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "ld < n"); }
  { Reacquire r = q; r.tick_stride = 99; CHECK(!refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "stride in (0, ld)"); }
  { Reacquire r = q; r.tick_stride = -100; CHECK(!refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "negative stride"); }
  { Reacquire r = q; r.tick_stride = 0; CHECK(refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "stride 0 overwrites"); }
  { Reacquire r = q; r.ring = -1; CHECK(!refused([&] { check_reacquire(r, 300.0, 100, false, true); }).empty(), "negative ring"); }
  CHECK(!refused([&] { check_reacquire(q, 300.0, 100, true, true); }).empty(), "a batch that keeps measured poses");
  CHECK(!refused([&] { check_reacquire(q, 300.0, 100, false, false); }).empty(), "a batch without its initial covariances");
  // rows, rings, keys
  q.tick_stride = 128; q.ring = 0;
  CHECK(q.row(5) == row + 5 * 128, "linear rows");
  q.ring = 3;
  CHECK(q.row(5) == row + 2 * 128 && q.row(3) == row, "ring rows");
  q.tick_stride = 0;
  CHECK(q.row(7) == row, "one row");
  { Reacquire r = q; CHECK(q.same(r), "same"); r.k = 4; CHECK(!q.same(r), "keyed by K"); r = q; r.event = row + 1; CHECK(!q.same(r), "keyed by the rows");
    r = q; r.ring = 4; CHECK(!q.same(r), "keyed by the ring"); r = q; r.tick_stride = 8; CHECK(!q.same(r), "keyed by the stride"); r = q; r.on = false; CHECK(!q.same(r), "keyed by on"); }
  { Reacquire r; CHECK(r.row(3) == nullptr, "no rows"); }
}

// A batch's slot -> row vector under append / erase as batch_store.cpp keeps it, with a simulated device row that only sees
// what the dirty range uploads; and its table of rows.
struct Model {
  std::vector<int> host, dev;   // slot_p0_ and its device copy
  DirtySlots dirty;
  long table_rows = 0;
  P0TableMirror tab;
  std::vector<int> dev_table;   // row ids the device table holds
  void append(long count, int row) {
    const long first = (long)host.size();
    host.insert(host.end(), (size_t)count, row);
    if (row + 1 > table_rows) table_rows = row + 1;
    if ((long)dev.size() < (long)host.size()) { dev.resize(host.size() * 2, -7); dirty.clear(); dirty.mark(0, (long)dev.size()); }   // reserve(): a new row
    dirty.mark(first, count);
  }
  void erase(long slot) {   // Batch::erase_slot
    const long last = (long)host.size() - 1;
    if (slot != last) { host[(size_t)slot] = host[(size_t)last]; dirty.mark(slot, 1); }
    host.pop_back();
  }
  void erase_many(const std::vector<int>& slots) {   // Batch::erase_slots: survivors from the tail fill the holes in order
    const long n = (long)host.size(), new_n = n - (long)slots.size();
    std::vector<char> gone((size_t)n, 0);
    for (int s : slots) gone[(size_t)s] = 1;
    long tail = new_n;
    for (long hole = 0; hole < new_n; ++hole) {
      if (!gone[(size_t)hole]) continue;
      while (gone[(size_t)tail]) ++tail;
      host[(size_t)hole] = host[(size_t)tail]; dirty.mark(hole, 1);
      ++tail;
    }
    host.resize((size_t)new_n);
  }
  void prepare() {   // Batch::prepare_reacquire
    const P0TableMirror::Upload u = tab.plan(table_rows);
    if (u.grow) dev_table.assign((size_t)u.new_cap, -1);
    for (long r = 0; r < u.count; ++r) dev_table[(size_t)(u.first + r)] = (int)(u.first + r);
    dirty.clip((long)host.size());
    for (long s = dirty.lo; s < dirty.hi; ++s) dev[(size_t)s] = host[(size_t)s];
    dirty.clear();
  }
  bool current() const {
    for (size_t s = 0; s < host.size(); ++s)
      if (dev[s] != host[s] || host[s] >= (int)dev_table.size() || dev_table[(size_t)host[s]] != host[s]) return false;
    return true;
  }
};

static void bookkeeping() {
  Model b;
  b.append(100, 0);
  b.prepare();
  CHECK(b.current() && b.tab.rows == 1 && b.dirty.empty(), "after the first append");
  { const P0TableMirror::Upload u = b.tab.plan(1); CHECK(!u.grow && u.count == 0, "nothing to upload twice"); }
  b.append(30, 1);       // a second initial covariance: the table grows, the new slots are uploaded
  b.append(1, 2);
  CHECK(!b.current(), "not current before prepare");
  b.prepare();
  CHECK(b.current() && b.tab.rows == 3 && b.tab.cap >= 3, "after two more appends");
  b.erase(5);            // the last slot (row 2) moves into slot 5
  CHECK(b.host[5] == 2 && b.host.size() == 130, "single erase moved the last slot");
  b.erase((long)b.host.size() - 1);   // the last slot itself: no move
  b.prepare();
  CHECK(b.current(), "after single erases");
  b.erase_many({0, 1, 2, 127, 128, 60});   // holes 0, 1, 2, 60 below the new size 123; 127, 128 in the tail
  CHECK(b.host.size() == 123 && b.host[0] == 1 && b.host[60] == 1, "batched erase filled the holes from the tail");
  b.prepare();
  CHECK(b.current(), "after a batched erase");
  b.append(500, 1);      // growth: a new device row, everything uploaded again
  b.prepare();
  CHECK(b.current(), "after growth");
  for (int k = 3; k < 40; ++k) b.append(2, k);   // the table grows geometrically and is uploaded whole when it does
  b.erase_many({3, 4, 5});
  b.prepare();
  CHECK(b.current() && b.tab.rows == 40 && b.tab.cap >= 40, "after many rows");
  DirtySlots d;
  CHECK(d.empty(), "starts empty");
  d.mark(10, 0); CHECK(d.empty(), "an empty mark");
  d.mark(10, 2); d.mark(3, 1); CHECK(d.lo == 3 && d.hi == 12, "the hull");
  d.clip(5); CHECK(d.lo == 3 && d.hi == 5, "clipped");
  d.clip(2); CHECK(d.empty(), "clipped away");
}

int main() {
  plan_rows();
  policy_checks();
  bookkeeping();
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("reacquire plan host test ok\n");
  return 0;
}
