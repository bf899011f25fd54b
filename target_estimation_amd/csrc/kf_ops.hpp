// kf_ops.hpp -- type-erased launch table: one Ops per (model, precision, lanes-per-target).
// The four kf_model_*.hip translation units instantiate the kernels; the host side
// (batch_store.cpp) only sees this table.
#pragma once
#include <hip/hip_runtime.h>

#include "kf_aux.hpp"
#include "te_layout.hpp"

namespace te {

struct StepParams {
  char* rec;
  char* rec_out = nullptr;        // dense single-tick launches: write the records here instead of in place (StepArgs::rec_out)
  const void* qr;                 // one [Q | R] block, or (cls != null) a table of them
  const int* cls = nullptr;       // per-slot parameter class: selects the per-class kernels
  long n;
  const int* idx;                 // non-null selects the indexed kernel
  const void* meas;               // SoA [7][meas_ld] in the batch precision, or null (predict only)
  long meas_ld;
  const unsigned char* has_meas;
  const double* dt_per;
  double dt;
  TClock* t_base;
  int* nm_base;
  int n_ticks = 1;        // > 1: temporally fused launch (state stays in registers for n_ticks ticks)
  long tick_stride = 0;   // elements between the measurement blocks of consecutive ticks
  long has_stride = 0;
  // fused own-time sphere query (dense single-tick launches): q_delta != null selects it
  double q_origin[3] = {0, 0, 0};
  double q_radius = 0;
  double* q_delta = nullptr;
  double* q_pose = nullptr;
  int nt_meas = 0;        // nontemporal measurement loads (kf_step.hpp StepArgs::nt_meas)
  int reverse = 0;        // walk the tiles last-to-first (zig-zag between consecutive ticks: kf_step.hpp StepArgs)
  // indexed launches: also write the per-slot getter table and a completion flag (StepArgs::o_pose); more than L.tpw entries
  // need done_count (a device word, zero between launches)
  double* o_pose = nullptr;
  double* o_twist = nullptr;
  double* o_acc = nullptr;
  int* done_flag = nullptr;
  int done_seq = 0;
  int* done_count = nullptr;
  // resident ("live") launch: live_posted != null (kf_step.hpp StepArgs::live_*); n_ticks = the most ticks it will serve
  const long long* live_posted = nullptr;
  long long* live_mirror = nullptr;
  int* live_progress = nullptr;
  int* live_done = nullptr;
  long live_ring = 0, live_first = 0;
  unsigned live_spin_limit = 0;
  unsigned long long live_idle_ticks = 0;
  int live_flags = 0;
  double* live_pose = nullptr;   // SoA [7][live_pose_ld] per-tick pose output of a live launch, or null
  long live_pose_ld = 0;
  // per-tick pose stream of a dense launch (StepArgs::pose): tick s of the launch writes SoA [7][pose_ld] doubles at
  // pose + (pose_ring > 0 ? s % pose_ring : s) * pose_tick_stride; null = none.  Layouts without a POSE kernel get a pose-writer
  // launch (outputs_kernel, OutArgs::pose_soa) behind every tick instead (OpsImpl::step).
  double* pose = nullptr;
  long pose_ld = 0;
  long pose_tick_stride = 0;
  long pose_ring = 0;
  // uniform tiles (StepArgs::tile_blk / tile_uni / promote): null / 0 for every launch but the dense ticks of a batch that keeps them
  double* tile_blk = nullptr;
  int* tile_uni = nullptr;
  int promote = 0;
  // innovation stream of a dense single tick (StepArgs::nis): this tick's NIS row [n] and, or null, its innovation block
  // [m][innov_ld].  The separable layouts of one-class batches write it from the step kernel (INNOV variants, in place, no fused
  // query); every other layout gets one innovation-writer launch (innov_kernel) BEFORE the step (OpsImpl::step).
  double* nis = nullptr;
  double* innov = nullptr;
  long innov_ld = 0;
  // The validation gate of a dense single tick with an innovation stream: gate > 0 (+inf included) accepts a measurement iff
  // (double)NIS <= gate; a rejected one is a tick without a measurement (state, covariance, unwrap memory, counter), its NIS and
  // innovation still reported.  0: none.  The separable layouts of one-class batches decide inside the step kernel (GATE,
  // kf_step_sep.hpp); every other layout's innovation writer is followed by the effective mask from its NIS row (gate_mask_kernel)
  // in gate_row [n] (the batch's own row), which the plain step kernel then takes as its has_meas.  gate_by_writer: take that path whatever the layout.
  // A gated tick always counts its accepted measurements in nm_base.
  double gate = 0.0;
  unsigned char* gate_row = nullptr;
  int gate_by_writer = 0;
  // Re-acquisition behind a gated dense single tick (ReacquireArgs below; kf_reacquire_impl.hpp): reacq = 1 puts one
  // reacquire_kernel launch behind the tick's step and ahead of its pose writer.  It keeps every slot's rejection run in
  // reacq_run [n], writes the tick's event bytes to reacq_event [>= n] (or null) and, with reacq_k > 0, re-initialises a slot
  // from this tick's measurement on its reacq_k-th consecutive rejection, P0 = reacq_p0 + reacq_p0_idx[slot] * N*N.  Needs the
  // gate; a tick without measurements launches nothing.
  int reacq = 0;
  int reacq_k = 0;
  unsigned char* reacq_run = nullptr;
  unsigned char* reacq_event = nullptr;
  const double* reacq_p0 = nullptr;
  const int* reacq_p0_idx = nullptr;
  // The by-id update policy (target_manager_set_update_gate) of an INDEXED single tick: gate_id = 1 with gate > 0 and a by-entry
  // NIS row in `nis` selects the gated indexed kernel (kf_step_sep.hpp, kf_step_sep_gate_indexed_kernel) -- ONE launch, the getter
  // table included when o_pose is set.  gate_id_k: -1 = gate only; 0..127 = the rejection runs in reacq_run (by slot) by
  // target_reacquire_c's table, re-initialising on the k-th consecutive rejection (k > 0) with P0 = reacq_p0 + reacq_p0_idx[slot] * N*N;
  // gate_id_event [n] (or null): this call's event bytes by entry.  reacq stays 0: no reacquire launch.
  int gate_id = 0;
  int gate_id_k = -1;
  unsigned char* gate_id_event = nullptr;
  // The gate INSIDE a resident launch (target_batch_live_set_gate; kf_step_sep.hpp, LiveGate): live_gate = 1 with live_posted
  // selects the gated resident kernel (kf_step_sep_live_gate_kernel).  Tick k of the session writes its NIS row at live_gate_nis +
  // (ring > 0 ? k % ring : k) * stride and, with live_gate_event, its event row likewise.  live_gate_k: -1 = gate only; 0..127 = the
  // rejection runs, read from reacq_run when the session starts and written back when its kernel leaves, re-initialising on the
  // k-th consecutive rejection (k > 0) with P0 = reacq_p0 + reacq_p0_idx[slot] * N*N.  gate / nis / reacq / gate_id stay 0.
  int live_gate = 0;
  double live_gate_nis_max = 0.0;
  double* live_gate_nis = nullptr;
  long live_gate_nis_stride = 0, live_gate_nis_ring = 0;
  int live_gate_k = -1;
  unsigned char* live_gate_event = nullptr;
  long live_gate_event_stride = 0, live_gate_event_ring = 0;
  // The gate INSIDE a launched fused call (target_batch_step_fused_gated; kf_step_sep.hpp, FusedGate): fused_gate = 1 on a dense
  // request in place of n_ticks >= 1 ticks.  Tick s of the call writes its NIS row at fused_gate_nis + (ring > 0 ? s % ring : s) *
  // stride, with fused_gate_innov its innovation block [m][fused_gate_innov_ld] likewise (the rows' ring) and with fused_gate_event its
  // event row (its own ring).  fused_gate_nis_max: 0 = no gate (the plain innovation stream), > 0 = gated.  fused_gate_k: -1 = no
  // policy; 0..127 = the rejection runs in reacq_run, re-initialising on the k-th consecutive rejection (k > 0) with P0 = reacq_p0 +
  // reacq_p0_idx[slot] * N*N.  gate / nis / reacq / gate_id / live_gate stay 0.  One launch where the layout has the kernel
  // (Ops::fused_gate and one (Q, R) class, no pose stream in the call); otherwise OpsImpl::step runs the ticks as single gated
  // requests (gate_row as for those) -- same results.
  int fused_gate = 0;
  double fused_gate_nis_max = 0.0;
  double* fused_gate_nis = nullptr;
  long fused_gate_nis_stride = 0, fused_gate_nis_ring = 0;
  double* fused_gate_innov = nullptr;
  long fused_gate_innov_ld = 0, fused_gate_innov_stride = 0;
  int fused_gate_k = -1;
  unsigned char* fused_gate_event = nullptr;
  long fused_gate_event_stride = 0, fused_gate_event_ring = 0;
  // The time-step schedule of a launched fused call (target_batch_step_fused_dt; kf_step_sep.hpp, DTTAB): dt_sched = 1 on a dense
  // request in place of n_ticks >= 1 ticks, plain or with fused_gate.  Tick s of the call runs with dt_host[s]; dt_tab holds the same
  // n_ticks doubles in device memory, written on the launch's stream ahead of it, and `dt` is not read.  One launch where the layout
  // has the kernel (Ops::fused_dt / fused_gate_dt, one (Q, R) class, no pose stream in the call); otherwise OpsImpl::step runs the
  // ticks as single requests with dt = dt_host[s] -- same results.
  int dt_sched = 0;
  const double* dt_host = nullptr;
  const double* dt_tab = nullptr;
};

// The launch behind a gated tick that keeps the rejection runs and re-initialises lost targets (kf_reacquire_impl.hpp).
struct ReacquireArgs {
  char* rec;                       // the records the tick's step has just written
  long n;
  const void* meas;                // the tick's SoA [7][meas_ld] block in the batch precision (never null: no launch without one)
  long meas_ld;
  const unsigned char* has_meas;   // the tick's per-slot mask as the caller gave it, or null
  const double* nis;               // the tick's NIS row [n], just written
  double gate;
  int k;                           // 0: count only
  unsigned char* run;              // [n] rejection runs
  unsigned char* event;            // [>= n] this tick's event bytes, or null
  const double* p0_tab;            // [rows][N*N] initial covariances
  const int* p0_idx;               // [n] row of every slot
  double* tile_blk;                // the batch's uniform tiles (null: none)
  int* tile_uni;
};

inline ReacquireArgs make_reacquire_args(const StepParams& p) {
  ReacquireArgs a;
  a.rec = p.rec_out ? p.rec_out : p.rec; a.n = p.n; a.meas = p.meas; a.meas_ld = p.meas_ld; a.has_meas = p.has_meas;
  a.nis = p.nis; a.gate = p.gate; a.k = p.reacq_k; a.run = p.reacq_run; a.event = p.reacq_event;
  a.p0_tab = p.reacq_p0; a.p0_idx = p.reacq_p0_idx; a.tile_blk = p.tile_blk; a.tile_uni = p.tile_uni;
  return a;
}

struct Ops {
  LayoutInfo L;
  int wpb;  // wavefronts per workgroup of the step kernel
  void (*step)(const StepParams&, hipStream_t);
  // wavefronts of the live kernel the device can hold at once (0: this (model, precision, layout) has no live kernel)
  // resident wavefronts of the plain (0) / the query-and-pose-output (1) / the gated (2: kf_step_sep_live_gate_kernel) variant
  long (*live_capacity)(int with_outputs);
  void (*init)(const InitArgs&, hipStream_t);
  // tile_blk / tile_uni: the batch's uniform tiles, honoured read-only (null: none)
  void (*get_state)(char* rec, const int* idx, long n, double* x, double* P, const double* tile_blk, const int* tile_uni, hipStream_t);
  void (*set_state)(char* rec, const int* idx, long n, const double* x, const double* P, const double* uw, hipStream_t);
  void (*move_record)(char* rec, long src, long dst, TClock* t_base, int* nm_base, int* cls, hipStream_t);
  void (*move_records)(char* rec, const int* src_dev, const int* dst_dev, long m, TClock* t_base, int* nm_base, int* cls, hipStream_t);
  void (*outputs)(const OutArgs&, hipStream_t);
  void (*pack_meas)(const double* aos, long n, void* soa, long ld, hipStream_t);
  void (*intersect)(const IntersectArgs&, hipStream_t);
  void (*outputs_rows)(const OutArgs&, hipStream_t);   // outputs_rows_kernel: poses at OutArgs::row_of_slot
  void (*innov)(const InnovArgs&, hipStream_t);       // innov_kernel: the innovations a tick WOULD see, records read-only
  // the same, then gate_mask_kernel: has_eff[e] = has && nis[e] <= gate for the step that follows
  void (*innov_gate)(const InnovArgs&, double gate, unsigned char* has_eff, hipStream_t);
  // shared-axes storage form only (L.shared_axes; null otherwise): write the n records of `rec` as plain LAYOUT_SEPARABLE_PACKED
  // records into `rec_plain` (a zero-filled buffer of the plain form's tiles), every kind's block copied to each of its axes
  void (*expand)(char* rec, char* rec_plain, long n, hipStream_t) = nullptr;
  // uniform tiles (L.lin_words > 0; null otherwise): write every flagged tile's block back into the linear P words of its n-bounded
  // lanes -- an exact copy; the caller clears the flags behind it
  void (*settle)(char* rec, long n, const double* tile_blk, const int* tile_uni, hipStream_t) = nullptr;
  // reacquire_kernel (kf_reacquire_impl.hpp) behind a gated tick: rejection runs, event bytes, re-initialisation
  void (*reacquire)(const ReacquireArgs&, hipStream_t) = nullptr;
  // 1: this (model, precision, layout) has a launched fused gated kernel (kf_step_sep_fused_gate_kernel); 0: a fused gated request
  // is served tick by tick
  int fused_gate = 0;
  // 1: ... has the launched fused kernel with a time-step table, plain (kf_step_sep_fused_dt_kernel) / gated
  // (kf_step_sep_fused_gate_dt_kernel); 0: a fused request with a schedule is served tick by tick
  int fused_dt = 0;
  int fused_gate_dt = 0;
};

// g == 0 selects the default lanes-per-target of the (model, precision); nullptr if unsupported
const Ops* get_ops(int type, int dtype, int g);
const Ops* get_ops_uv(int dtype, int g);
const Ops* get_ops_ua(int dtype, int g);
const Ops* get_ops_ar(int dtype, int g);
const Ops* get_ops_av(int dtype, int g);
// the shared-axes storage form of the separable layout with packed groups (lanes code kLanesSeparableShared, fp64)
const Ops* get_ops_shared_uv();
const Ops* get_ops_shared_ua();
const Ops* get_ops_shared_ar();
const Ops* get_ops_shared_av();

}  // namespace te
