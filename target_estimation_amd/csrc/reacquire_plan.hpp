// reacquire_plan.hpp -- host-only, no HIP: the re-acquisition policy of a gated call (target_batch_c.h, target_reacquire_c), what
// is refused about it, and the bookkeeping of the two device tables its kernel reads -- the batch's distinct initial covariances
// and the row of every slot (batch_store.cpp keeps them; tests/host/reacquire_plan_host_test.cpp builds this header alone).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>

namespace te {

// K and the per-tick event rows: after tick s of a call, row b = (ring > 0 ? s % ring : s) at event + b * tick_stride holds one
// byte per slot (column): 0 = no measurement or accepted, c' = rejected (the run it reached), 0x80 | c' = rejected and
// re-initialised.  tick_stride 0: every tick overwrites one row.  event == null: no rows.
struct Reacquire {
  bool on = false;
  int k = 0;                       // 1..127: re-initialise on the k-th consecutive rejection; 0: count only
  unsigned char* event = nullptr;
  long ld = 0;
  long tick_stride = 0;
  long ring = 0;
  unsigned char* row(long s) const { return event ? event + (ring > 0 ? s % ring : s) * tick_stride : nullptr; }
  bool same(const Reacquire& o) const {   // (recorded graphs are keyed by the policy as well)
    return on == o.on && k == o.k && event == o.event && ld == o.ld && tick_stride == o.tick_stride && ring == o.ring;
  }
};

// throws std::invalid_argument unless the policy can be served: gate = the call's nis_max, n = the batch size
inline void check_reacquire(const Reacquire& q, double gate, long n, bool keeps_measured_poses, bool p0_kept) {
  if (!q.on) return;
  const std::string pre = "target_estimation_amd: re-acquisition: ";
  if (!(gate > 0.0)) throw std::invalid_argument(pre + "a policy needs the gate (nis_max > 0): it counts the gate's rejections");
  if (q.k < 0 || q.k > 127) throw std::invalid_argument(pre + "max_rejects must be 0..127, got " + std::to_string(q.k));
  if (q.event) {
    if (q.ld < n) throw std::invalid_argument(pre + "event rows: ld " + std::to_string(q.ld) + " < batch size " + std::to_string(n));
    if (q.tick_stride < 0 || (q.tick_stride > 0 && q.tick_stride < q.ld)) throw std::invalid_argument(pre + "event rows: tick_stride must be 0 or >= ld");
    if (q.ring < 0) throw std::invalid_argument(pre + "event rows: negative ring_ticks");
  }
  if (keeps_measured_poses) throw std::invalid_argument(pre + "not served for a batch that keeps measured poses (set_keep_measurement)");
  if (!p0_kept) throw std::invalid_argument(pre + "the batch no longer keeps its initial covariances (too many distinct ones)");
}

// The update policy of the by-id paths (target_manager_c.h, target_manager_set_update_gate): sticky, per manager and model, off
// by default.  nis_max 0 = no gate, > 0 (+inf included) = a measurement is folded in iff (double)NIS <= nis_max.  max_rejects -1 =
// gate only (the rejection runs are neither read nor written), 0 = count only, 1..127 = re-initialise on the K-th consecutive
// rejection, by the table of Reacquire above.
struct UpdateGate {
  double nis_max = 0.0;
  int max_rejects = -1;
  bool on() const { return nis_max > 0.0; }
  bool runs() const { return on() && max_rejects >= 0; }
};
// throws std::invalid_argument for the policies that are refused whatever the batch
inline void check_update_gate(double nis_max, int max_rejects) {
  const std::string pre = "target_estimation_amd: update gate: ";
  if (!(nis_max >= 0.0)) throw std::invalid_argument(pre + "nis_max must be 0 (no gate) or positive");
  if (max_rejects < -1 || max_rejects > 127) throw std::invalid_argument(pre + "max_rejects must be -1..127, got " + std::to_string(max_rejects));
  if (max_rejects >= 0 && !(nis_max > 0.0)) throw std::invalid_argument(pre + "max_rejects >= 0 needs the gate (nis_max > 0): it counts the gate's rejections");
}

// The device copy of the host table of distinct initial covariances (rows are only ever appended): what to do before a launch
// reads it.  grow: allocate new_cap rows, copy nothing over -- every row is uploaded again (first = 0).
struct P0TableMirror {
  long rows = 0;   // rows the device holds
  long cap = 0;    // rows allocated
  struct Upload { bool grow; long new_cap; long first; long count; };
  Upload plan(long host_rows) {
    Upload u{false, cap, rows, host_rows - rows};
    if (host_rows > cap) { u.grow = true; u.new_cap = std::max(host_rows, 2 * cap); u.first = 0; u.count = host_rows; cap = u.new_cap; }
    rows = host_rows;
    return u;
  }
  void reset() { rows = 0; cap = 0; }
};

// The device copy of the slot -> row index: the host vector is the truth, append / erase mark the slots they wrote, and one copy
// of [lo, hi) brings the device row up to date before a launch reads it.
struct DirtySlots {
  long lo = 0, hi = 0;   // empty when lo >= hi
  bool empty() const { return lo >= hi; }
  void mark(long first, long count) {
    if (count <= 0) return;
    if (empty()) { lo = first; hi = first + count; }
    else { lo = std::min(lo, first); hi = std::max(hi, first + count); }
  }
  // the batch shrank to n slots: nothing beyond them is read
  void clip(long n) { hi = std::min(hi, n); if (empty()) clear(); }
  void clear() { lo = hi = 0; }
};

}  // namespace te
