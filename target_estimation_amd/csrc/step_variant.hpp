// step_variant.hpp -- which step kernels exist and which launches serve a request.  Plain C++17 without a HIP dependency
// (tests/host/step_variant_host_test.cpp compiles it with g++).
//
// The three step kernels (kf_step_sep_kernel / sep_step_wave, kf_step_kernel, kf_step_population_kernel) take their variant as ONE
// unsigned template argument made of the named bits below; kf_step.hpp and kf_step_sep.hpp say what each bit compiles in.
// sep_variant_ok / dense_variant_ok are the single statement of which combinations make sense (each kernel static_asserts its
// own), kSepVariants / kDenseVariants the ones the library ships, variant_shipped the per-layout exclusions, and plan_step the
// launches of one OpsImpl::step request.  DESIGN.md ("Step-kernel variants") says how a new variant is added.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

namespace te {

enum StepVariantBit : unsigned {
  kIndexed = 1u << 0,   // StepParams::idx: the entries' slots come from a list
  kFused = 1u << 1,     // n_ticks > 1 in one launch, the state stays in registers
  kQuery = 1u << 2,     // the own-time sphere query behind the tick (q_delta)
  kPerQR = 1u << 3,     // Q and R of the target's own parameter class (cls)
  kAB = 1u << 4,        // an A -> B tick (rec_out)
  kPose = 1u << 5,      // the per-tick pose stream from the step kernel (pose)
  kInnov = 1u << 6,     // the innovation stream from the step kernel (nis)
  kLive1 = 1u << 7,     // the live field (two bits): 1 = resident launch,
  kLive2 = 2u << 7,     //                            2 = resident launch with the per-tick query / pose output
};
constexpr unsigned kLiveMask = 3u << 7, kVariantBits = 9;
constexpr int sv_live(unsigned v) { return (int)((v & kLiveMask) >> 7); }
constexpr bool sv_has(unsigned v, unsigned bit) { return (v & bit) != 0; }

// kf_step_sep_kernel / sep_step_wave; shared_layout: the shared-axes storage form (LAYOUT_SEPARABLE_SHARED)
constexpr bool sep_variant_ok(unsigned v, bool shared_layout) {
  const bool INDEXED = sv_has(v, kIndexed), FUSED = sv_has(v, kFused), QUERY = sv_has(v, kQuery), PERQR = sv_has(v, kPerQR), AB = sv_has(v, kAB),
             POSE = sv_has(v, kPose), INNOV = sv_has(v, kInnov);
  const int LIVE = sv_live(v);
  return v < (1u << kVariantBits) && LIVE != 3 &&
         // the innovation stream is an output of single ticks in place of one-class batches: of the dense ones and, with kIndexed, of
         // the gated by-id step (kf_step_sep_gate_indexed_kernel), whose NIS row is indexed by entry.  kSepVariants does not list the
         // latter: no plain kInnov | kIndexed kernel is shipped, plan_step reaches the gated one through StepPlan::gate_by_id.
         (!INNOV || (!FUSED && !QUERY && !PERQR && !LIVE && !AB && !POSE)) &&
         // the pose stream is an output of dense launches of one-class batches
         (!POSE || (!INDEXED && !PERQR && !LIVE)) &&
         // A -> B ticks are dense single-tick launches without the fused query
         (!AB || (!INDEXED && !FUSED && !QUERY && !LIVE)) &&
         // the fused query is for dense single-tick launches
         !(QUERY && (INDEXED || FUSED)) &&
         // per-class Q/R: single-tick launches without the fused query
         !(PERQR && (FUSED || QUERY)) &&
         // live launches are dense multi-tick launches
         (!LIVE || (FUSED && !INDEXED && !QUERY && !PERQR)) &&
         // the shared-axes storage form: single-tick launches of one-class batches (the host expands the batch first)
         (!shared_layout || (!FUSED && !PERQR && !LIVE));
}
// kf_step_kernel: no resident launches and no output streams (pose-writer / innovation-writer launches serve those)
constexpr bool dense_variant_ok(unsigned v) {
  const bool INDEXED = sv_has(v, kIndexed), FUSED = sv_has(v, kFused), QUERY = sv_has(v, kQuery), PERQR = sv_has(v, kPerQR), AB = sv_has(v, kAB);
  return (v & ~(kIndexed | kFused | kQuery | kPerQR | kAB)) == 0 && (!AB || (!INDEXED && !FUSED && !QUERY)) && !(QUERY && (INDEXED || FUSED)) &&
         !(PERQR && (FUSED || QUERY));
}
// kf_step_population_kernel: dense single ticks of one-class batches
constexpr bool population_variant_ok(unsigned v, bool shared_layout) {
  return (v & ~(kQuery | kAB | kPose | kInnov)) == 0 && sep_variant_ok(v, shared_layout);
}

// kf_step_population_fused_kernel<T, GATE, DTTAB>: the launched fused loops (variant word kFused; the gate and the table are template
// arguments next to it, as for the per-batch kernels) on the population grid, plain form of the separable layout with packed
// groups.  An instantiation that would need scratch is not shipped -- its requests are served per batch -- and is listed here
// (profiles/fused_all_kernel_resources.txt).  None is.
constexpr bool population_fused_ok(bool f64, bool gated, bool dt_table) {
  (void)f64; (void)gated; (void)dt_table;
  return sep_variant_ok(kFused, false);
}

// The ONE argument of kf_step_population_fused_kernel: per part what the per-batch gated kernel with a time-step table finds at
// offset 0 of its kernel-argument segment (Seg = FusedGateDtSegment<T>, kf_step_sep.hpp), then the grid split.  The gated loop of
// part k reads its arguments at the compile-time offset population_fused_seg_offset<Seg>(k) of the segment; the whole struct must
// stay within the 4 KB a kernel's arguments may take.
template <class Seg>
struct PopulationFusedLayout {
  Seg part[4];       // indexed by ModelType
  unsigned end[4];   // first workgroup BEHIND part k (cumulative; an absent model has end[k] == end[k - 1])
};
template <class Seg>
constexpr unsigned population_fused_seg_offset(int k) {
  return (unsigned)(sizeof(Seg) * (unsigned)k);   // (part is the first member: offset 0, asserted where the kernel is)
}
template <class Seg>
constexpr bool population_fused_args_fit() {
  return sizeof(PopulationFusedLayout<Seg>) <= 4096;
}

// Who serves a fused replay of a whole manager's shard (Shard::stepFusedAll): ONE launch of kf_step_population_fused_kernel -- the
// plain loop or the gated one -- or the per-batch calls in batch order inside the same call (same bits, their launch counts).
struct FusedAllBatch {
  long n = 0;                // targets (0: the batch takes no part)
  int type = 0;              // ModelType
  bool ready = false;        // separable layout with packed groups, one (Q, R) class (Batch::population_ready; the storage form does
                             // not matter: a shared-axes batch is expanded ahead of every fused call)
  bool keep_meas = false;    // keeps measured-pose rows
  bool pose = false;         // a pose stream in the call
  bool nis = false;          // NIS rows in the call
  bool gate_or_policy = false;   // nis_max > 0 or a re-acquisition policy in the call
};
enum class FusedAllRoute { kPerBatch, kPlainLoop, kGatedLoop };
// population_tick: ShardSettings::population_tick; max_table_ticks: kDtTabMaxTicks (dt_schedule.hpp)
constexpr FusedAllRoute plan_fused_all(bool population_tick, bool f64, const FusedAllBatch* b, long nb, bool scheduled, long n_ticks, long max_table_ticks) {
  if (!population_tick) return FusedAllRoute::kPerBatch;
  bool seen[4] = {false, false, false, false};
  int present = 0, with_nis = 0;
  bool anything = false;
  for (long i = 0; i < nb; ++i) {
    if (b[i].n <= 0) continue;
    if (!b[i].ready || b[i].keep_meas || b[i].pose || b[i].type < 0 || b[i].type > 3 || seen[b[i].type]) return FusedAllRoute::kPerBatch;
    seen[b[i].type] = true;
    ++present;
    with_nis += b[i].nis ? 1 : 0;
    anything = anything || b[i].nis || b[i].gate_or_policy;
  }
  if (present < 2) return FusedAllRoute::kPerBatch;
  if (scheduled && n_ticks > max_table_ticks) return FusedAllRoute::kPerBatch;
  // the plain loop: nothing to report or decide anywhere; the gated loop: every part has at least its NIS rows (a part's nis_max may
  // be 0: the plain stream).  A call in which only some batches carry streams is served per batch.
  if (!anything) return population_fused_ok(f64, false, scheduled) ? FusedAllRoute::kPlainLoop : FusedAllRoute::kPerBatch;
  if (with_nis != present) return FusedAllRoute::kPerBatch;
  return population_fused_ok(f64, true, scheduled) ? FusedAllRoute::kGatedLoop : FusedAllRoute::kPerBatch;
}

// The variants the library instantiates, before the per-layout exclusions of variant_shipped.
constexpr unsigned kSepVariants[] = {0, kIndexed, kFused, kQuery, kAB, kPose, kAB | kPose, kFused | kPose, kQuery | kPose, kInnov,
                                     kFused | kLive1, kFused | kLive2, kPerQR, kIndexed | kPerQR, kPerQR | kAB};
constexpr unsigned kDenseVariants[] = {0, kIndexed, kFused, kQuery, kAB, kPerQR, kIndexed | kPerQR, kPerQR | kAB};

// What OpsImpl<M, T, G, LAYOUT> knows about itself at compile time.
struct StepTraits {
  bool sep;                      // the axis-separable kernel (kf_step_sep_kernel), else the dense one (kf_step_kernel)
  bool shared;                   // the shared-axes storage form
  bool uniform_tiles;            // ... whose kernels carry uniform tiles
  bool has_live;                 // resident kernels exist (packed groups)
  bool fused_pose_tick_by_tick;  // no kFused | kPose kernel: it would cost a wavefront per SIMD or spill
  bool fused_spills;             // no kFused kernel (dense): it would spill
  int tpw;                       // targets per wavefront
  bool gate_by_writer = false;   // no gated kernel (it would spill or need scratch): the gate's mask comes from the innovation writer
  bool fused_gate_tick_by_tick = false;   // no launched fused gated kernel (it would need scratch): a fused gated request is served tick by tick
  // no launched fused kernel with a time-step table (it would need scratch): a fused request with a schedule is served tick by
  // tick -- the plain loop / the gated loop, each on its own
  bool fused_dt_tick_by_tick = false;
  bool fused_gate_dt_tick_by_tick = false;
};

template <unsigned N>
constexpr bool variant_in(const unsigned (&list)[N], unsigned v) {
  for (unsigned i = 0; i < N; ++i)
    if (list[i] == v) return true;
  return false;
}
constexpr bool variant_shipped(unsigned v, const StepTraits& t) {
  if (!t.sep) return variant_in(kDenseVariants, v) && dense_variant_ok(v) && !(sv_has(v, kFused) && t.fused_spills);
  return variant_in(kSepVariants, v) && sep_variant_ok(v, t.shared) && (sv_live(v) == 0 || t.has_live) &&
         !(v == (kFused | kPose) && t.fused_pose_tick_by_tick);
}

// The launches of one step request, in order: [innovation writer] then, once or (tick_by_tick) once per tick of the request,
// the step kernel `variant` [and the pose writer behind it].
struct StepPlan {
  bool innov_writer_first = false;
  bool tick_by_tick = false;
  unsigned variant = 0;
  bool pose_writer_after_each_tick = false;
  // the request carries a validation gate.  Without innov_writer_first the step is the gated kInnov kernel (kf_step_sep.hpp,
  // GATE: a template argument next to the variant word, not a bit of it); with it the innovation writer is followed by the mask
  // launch (gate_mask_kernel: has && nis <= gate from the NIS row just written), and the plain step kernel behind the two takes
  // that row as its has_meas: three launches per tick.
  bool gated = false;
  // the request keeps rejection runs / re-acquires (P::reacq): one reacquire launch behind the step of the (gated, measured) tick
  // and ahead of its pose writer
  bool reacquire_after_step = false;
  // the request carries the by-id update policy (P::gate_id): an indexed single tick, gated, served by ONE launch of the gated
  // indexed kernel (kf_step_sep_gate_indexed_kernel: variant kInnov | kIndexed, the rejection runs and the re-initialisation in
  // its tail, the getter table too when the request has one).  Never together with innov_writer_first / reacquire_after_step.
  bool gate_by_id = false;
  // the request is a resident launch with the gate inside the session (P::live_gate): the gated resident kernel
  // (kf_step_sep_live_gate_kernel), the variant word kFused | kLive2 and the gate a template argument next to it
  bool live_gated = false;
  // the request is a launched fused call with the gate, the innovation stream and the policy inside it (P::fused_gate).  Without
  // tick_by_tick: ONE launch of kf_step_sep_fused_gate_kernel for the whole call, the variant word kFused and the gate a template
  // argument next to it.  With tick_by_tick no such kernel serves the batch (the dense layouts, several (Q, R) classes, a pose
  // stream in the same call, StepTraits::fused_gate_tick_by_tick): the caller runs the call's ticks as single gated requests, each
  // planned on its own -- `variant` is then 0 and says nothing.
  bool fused_gated = false;
  // the request carries a time-step schedule (P::dt_sched) and ONE launch serves it: the kFused loop -- plain, or with fused_gated
  // the gated one -- whose tick s reads entry s of the device table P::dt_tab (kf_step_sep.hpp, DTTAB: a template argument next to
  // the variant word, not a bit of it).  A schedule request without it is tick_by_tick: the caller gives tick s the dt P::dt_host[s].
  bool dt_table = false;
};

// The gate of a request: P::gate (a double, 0 = none) and P::gate_by_writer (the caller asks for the writer's mask row) where the
// request type has them; a request type without them plans as it always did.
template <class P, class = void> struct has_gate_member : std::false_type {};
template <class P> struct has_gate_member<P, std::void_t<decltype(std::declval<const P&>().gate)>> : std::true_type {};
template <class P, class = void> struct has_gate_by_writer_member : std::false_type {};
template <class P> struct has_gate_by_writer_member<P, std::void_t<decltype(std::declval<const P&>().gate_by_writer)>> : std::true_type {};
template <class P>
constexpr double requested_gate(const P& p) {
  if constexpr (has_gate_member<P>::value) return (double)p.gate;
  else return 0.0;
}
template <class P, class = void> struct has_reacq_member : std::false_type {};
template <class P> struct has_reacq_member<P, std::void_t<decltype(std::declval<const P&>().reacq)>> : std::true_type {};
template <class P>
constexpr bool requested_reacquire(const P& p) {
  if constexpr (has_reacq_member<P>::value) return p.reacq != 0;
  else return false;
}
// The by-id update policy of a request: P::gate_id (non-zero = the request is a by-id update under a manager's policy; it then
// has P::gate_id_k, -1 = gate only, 0..127 as P::reacq_k, and the pointers P::reacq_run / reacq_p0 / reacq_p0_idx as well).
template <class P, class = void> struct has_gate_id_member : std::false_type {};
template <class P> struct has_gate_id_member<P, std::void_t<decltype(std::declval<const P&>().gate_id)>> : std::true_type {};
template <class P>
constexpr bool requested_gate_by_id(const P& p) {
  if constexpr (has_gate_id_member<P>::value) return p.gate_id != 0;
  else return false;
}
// The gate of a resident session: P::live_gate (non-zero = the launch is a resident one that gates inside its tick loop; the request
// then has P::live_gate_nis_max (> 0), the NIS rows P::live_gate_nis / _nis_stride / _nis_ring, P::live_gate_k (-1 = gate only, 0..127
// as P::reacq_k), the event rows P::live_gate_event / _event_stride / _event_ring and, for the runs, the pointers P::reacq_run /
// reacq_p0 / reacq_p0_idx).  A request type without the member plans as it always did.
template <class P, class = void> struct has_live_gate_member : std::false_type {};
template <class P> struct has_live_gate_member<P, std::void_t<decltype(std::declval<const P&>().live_gate)>> : std::true_type {};
template <class P>
constexpr bool requested_live_gate(const P& p) {
  if constexpr (has_live_gate_member<P>::value) return p.live_gate != 0;
  else return false;
}
// The gate of a launched fused call: P::fused_gate (non-zero = the request is target_batch_step_fused_gated's; it then has
// P::fused_gate_nis_max (>= 0; 0 = the plain innovation stream), the NIS rows P::fused_gate_nis / _nis_stride / _nis_ring, the innovation
// blocks P::fused_gate_innov / _innov_ld / _innov_stride (the rows' ring), P::fused_gate_k (-1 = no policy, 0..127 as P::reacq_k), the
// event rows P::fused_gate_event / _event_stride / _event_ring and, for the runs, the pointers P::reacq_run / reacq_p0 /
// reacq_p0_idx).  A request type without the member plans as it always did.
template <class P, class = void> struct has_fused_gate_member : std::false_type {};
template <class P> struct has_fused_gate_member<P, std::void_t<decltype(std::declval<const P&>().fused_gate)>> : std::true_type {};
template <class P>
constexpr bool requested_fused_gate(const P& p) {
  if constexpr (has_fused_gate_member<P>::value) return p.fused_gate != 0;
  else return false;
}
// The time-step schedule of a launched fused call: P::dt_sched (non-zero = the request is target_batch_step_fused_dt's: a dense request in
// place of n_ticks >= 1 ticks, plain or with P::fused_gate, whose tick s runs with dt[s]; it then has P::dt_host, the schedule on
// the host [n_ticks], and P::dt_tab, the same values in device memory, written on the stream ahead of the launch).  A request type
// without the member plans as it always did.
template <class P, class = void> struct has_dt_sched_member : std::false_type {};
template <class P> struct has_dt_sched_member<P, std::void_t<decltype(std::declval<const P&>().dt_sched)>> : std::true_type {};
template <class P>
constexpr bool requested_dt_sched(const P& p) {
  if constexpr (has_dt_sched_member<P>::value) return p.dt_sched != 0;
  else return false;
}
template <class P>
void check_dt_sched(const P& p, bool one_launch) {
  if constexpr (has_dt_sched_member<P>::value) {
    if (!p.dt_host) throw std::runtime_error("target_estimation_amd: the time-step schedule: a request carries it on the host");
    if (one_launch && !p.dt_tab) throw std::runtime_error("target_estimation_amd: the time-step schedule: one launch reads it from a device table");
  }
}
template <class P>
constexpr bool requested_gate_by_writer(const P& p) {
  if constexpr (has_gate_by_writer_member<P>::value) return p.gate_by_writer != 0;
  else return false;
}

// P: StepParams (kf_ops.hpp), or anything with its member names.
// Every bit a request asks for, before plan_step decides which launch serves it.
template <class P>
constexpr unsigned requested_variant(const P& p) {
  return (p.idx ? kIndexed : 0u) | (p.n_ticks > 1 ? kFused : 0u) | (p.q_delta ? kQuery : 0u) | (p.cls ? kPerQR : 0u) | (p.rec_out ? kAB : 0u) |
         (p.pose ? kPose : 0u) | (p.nis ? kInnov : 0u) | (p.live_posted ? kLive1 : 0u);
}
// Throws for the requests no launch sequence serves.
template <class P>
StepPlan plan_step(const StepTraits& t, const P& p) {
  StepPlan plan;
  const double gate = requested_gate(p);
  if (!(gate >= 0.0)) throw std::runtime_error("target_estimation_amd: the gate (nis_max) must be 0 (none) or positive");
  plan.gated = gate > 0.0;
  if constexpr (has_gate_id_member<P>::value) {
    if (requested_gate_by_id(p)) {   // the by-id policy: one launch of the gated indexed kernel, or refused
      const char* pre = "target_estimation_amd: the update gate by id: ";
      if (!plan.gated) throw std::runtime_error(std::string(pre) + "a policy needs the gate (nis_max > 0)");
      if (!p.idx || !p.nis) throw std::runtime_error(std::string(pre) + "an indexed launch with a by-entry NIS row");
      if (p.n_ticks > 1 || p.live_posted || p.rec_out || p.q_delta || p.pose || p.tile_uni || requested_reacquire(p) || requested_gate_by_writer(p))
        throw std::runtime_error(std::string(pre) + "a single indexed tick in place, without the dense calls' streams");
      if (p.gate_id_k < -1 || p.gate_id_k > 127) throw std::runtime_error(std::string(pre) + "max_rejects must be -1..127");
      if (p.gate_id_k >= 0 && (!p.reacq_run || !p.reacq_p0 || !p.reacq_p0_idx))
        throw std::runtime_error(std::string(pre) + "rejection runs need the batch's run row and its table of initial covariances");
      if (!t.sep || p.cls || t.gate_by_writer)
        throw std::runtime_error(std::string(pre) + "no gated indexed kernel for this batch (dense layouts, several (Q, R) classes)");
      if (p.o_pose && ((p.n > t.tpw && !p.done_count) || !p.o_twist || !p.o_acc || !p.done_flag))
        throw std::runtime_error("target_estimation_amd: the fused getter table needs an indexed launch (and a wavefront counter beyond one wavefront of entries)");
      plan.gate_by_id = true;
      plan.variant = kInnov | kIndexed;
      return plan;
    }
  }
  if constexpr (has_fused_gate_member<P>::value) {
    if (requested_fused_gate(p)) {   // the launched fused call with the gate inside: one launch, or tick by tick, or refused
      const char* pre = "target_estimation_amd: the fused gate: ";
      if (!(p.fused_gate_nis_max >= 0.0)) throw std::runtime_error(std::string(pre) + "nis_max must be 0 (none) or positive");
      if (!p.fused_gate_nis || p.fused_gate_nis_stride < 0 || p.fused_gate_nis_ring < 0)
        throw std::runtime_error(std::string(pre) + "it reports its decisions in NIS rows");
      if (p.fused_gate_innov && (p.fused_gate_innov_ld < p.n || p.fused_gate_innov_stride < 0)) throw std::runtime_error(std::string(pre) + "malformed innovation blocks");
      if (p.fused_gate_k < -1 || p.fused_gate_k > 127) throw std::runtime_error(std::string(pre) + "max_rejects must be -1..127");
      if (p.fused_gate_k >= 0 && !(p.fused_gate_nis_max > 0.0)) throw std::runtime_error(std::string(pre) + "a policy needs the gate (nis_max > 0)");
      if (p.fused_gate_k >= 0 && !p.reacq_run) throw std::runtime_error(std::string(pre) + "rejection runs need the batch's run row");
      if (p.fused_gate_k > 0 && (!p.reacq_p0 || !p.reacq_p0_idx)) throw std::runtime_error(std::string(pre) + "re-acquisition needs the batch's table of initial covariances");
      if (p.fused_gate_event && (p.fused_gate_k < 0 || p.fused_gate_event_stride < 0 || p.fused_gate_event_ring < 0))
        throw std::runtime_error(std::string(pre) + "event rows belong to a policy (max_rejects >= 0)");
      if (p.n_ticks < 1 || p.idx || p.live_posted || p.rec_out || p.q_delta || p.o_pose || p.tile_uni || t.shared)
        throw std::runtime_error(std::string(pre) + "a dense fused launch in place of a batch in the plain form");
      if (plan.gated || p.nis || requested_reacquire(p) || requested_gate_by_id(p) || requested_live_gate(p) || requested_gate_by_writer(p))
        throw std::runtime_error(std::string(pre) + "not together with the single ticks' gate, streams or policies");
      plan.fused_gated = true;
      plan.tick_by_tick = !t.sep || p.cls || p.pose || t.fused_gate_tick_by_tick || t.gate_by_writer;
      if (requested_dt_sched(p)) {   // the gated loop with the table, where it exists
        plan.tick_by_tick = plan.tick_by_tick || t.fused_gate_dt_tick_by_tick;
        plan.dt_table = !plan.tick_by_tick;
        check_dt_sched(p, plan.dt_table);
      }
      plan.variant = plan.tick_by_tick ? 0u : (unsigned)kFused;
      return plan;
    }
  }
  if (plan.gated && (!p.nis || p.idx || p.n_ticks > 1 || p.live_posted || p.o_pose))
    throw std::runtime_error("target_estimation_amd: the gate acts in dense single ticks with an innovation stream (its NIS row reports the decisions)");
  // (a request type with P::reacq has P::reacq_k, the pointers P::reacq_run / reacq_p0 / reacq_p0_idx and P::meas as well)
  if constexpr (has_reacq_member<P>::value) {
    if (requested_reacquire(p)) {
      if (!plan.gated) throw std::runtime_error("target_estimation_amd: re-acquisition needs the gate (nis_max > 0): it counts the gate's rejections");
      if (p.reacq_k < 0 || p.reacq_k > 127) throw std::runtime_error("target_estimation_amd: re-acquisition: max_rejects must be 0..127");
      if (!p.reacq_run || !p.reacq_p0 || !p.reacq_p0_idx)
        throw std::runtime_error("target_estimation_amd: re-acquisition needs the batch's rejection runs and its table of initial covariances");
      plan.reacquire_after_step = p.meas ? true : false;   // (a tick without measurements changes no run: no launch)
    }
  }
  // (Batch expands a shared-axes batch to the plain form before any of these: batch_store.cpp, demote_shared)
  if (t.shared && (p.live_posted || p.cls || p.n_ticks > 1))
    throw std::runtime_error("target_estimation_amd: the shared-axes storage form has single-tick kernels of one-class batches only");
  if (p.tile_uni && (!t.uniform_tiles || p.idx || !p.tile_blk))
    throw std::runtime_error("target_estimation_amd: uniform tiles are a property of dense ticks of the shared-axes storage form");
  if (requested_dt_sched(p)) {
    if (p.n_ticks < 1 || p.idx || p.live_posted || p.rec_out || p.q_delta || p.o_pose || p.nis || p.tile_uni || t.shared || plan.gated ||
        requested_reacquire(p) || requested_gate_by_id(p) || requested_live_gate(p))
      throw std::runtime_error("target_estimation_amd: the time-step schedule: a dense fused launch in place of a batch in the plain form");
  }
  if (requested_live_gate(p) && !p.live_posted)
    throw std::runtime_error("target_estimation_amd: the resident gate belongs to a live launch (live_posted)");
  if (p.live_posted) {   // a resident launch serves its ticks, query and poses by itself
    if (!t.has_live)
      throw std::runtime_error("target_estimation_amd: live mode needs the axis-separable layout with packed groups (the automatic choice for the shipped models)");
    if (p.idx || p.cls || p.rec_out || !p.live_progress || !p.live_mirror || !p.live_done || p.live_ring <= 0 || p.n_ticks < 1)
      throw std::runtime_error("target_estimation_amd: a live launch is a dense launch of a one-class batch over a measurement ring");
    plan.variant = kFused | ((p.q_delta || p.live_pose) ? kLive2 : kLive1);
    if constexpr (has_live_gate_member<P>::value) {
      if (requested_live_gate(p)) {   // the gated resident kernel: the pose / query session's loop with the gate inside, or refused
        const char* pre = "target_estimation_amd: the resident gate: ";
        if (!(p.live_gate_nis_max > 0.0)) throw std::runtime_error(std::string(pre) + "nis_max must be positive");
        if (!p.live_gate_nis || p.live_gate_nis_stride < 0 || p.live_gate_nis_ring < 0) throw std::runtime_error(std::string(pre) + "it reports its decisions in NIS rows");
        if (p.live_gate_k < -1 || p.live_gate_k > 127) throw std::runtime_error(std::string(pre) + "max_rejects must be -1..127");
        if (p.live_gate_k >= 0 && !p.reacq_run) throw std::runtime_error(std::string(pre) + "rejection runs need the batch's run row");
        if (p.live_gate_k > 0 && (!p.reacq_p0 || !p.reacq_p0_idx)) throw std::runtime_error(std::string(pre) + "re-acquisition needs the batch's table of initial covariances");
        if (p.live_gate_event && (p.live_gate_k < 0 || p.live_gate_event_stride < 0 || p.live_gate_event_ring < 0))
          throw std::runtime_error(std::string(pre) + "event rows belong to a policy (max_rejects >= 0)");
        if (p.nis || requested_reacquire(p) || requested_gate_by_id(p) || requested_gate_by_writer(p))
          throw std::runtime_error(std::string(pre) + "not together with the launched calls' gate, streams or policies");
        plan.variant = kFused | kLive2;
        plan.live_gated = true;
      }
    }
    return plan;
  }
  if (p.o_pose && (!p.idx || (p.n > t.tpw && !p.done_count) || !p.o_twist || !p.o_acc || !p.done_flag))
    throw std::runtime_error("target_estimation_amd: the fused getter table needs an indexed launch (and a wavefront counter beyond one wavefront of entries)");
  if (p.nis && (p.idx || p.o_pose || p.n_ticks > 1 || p.rec_out || p.q_delta))
    throw std::runtime_error("target_estimation_amd: the innovation stream is an output of dense single ticks in place, without the fused query");
  if (p.pose && (p.idx || p.o_pose)) throw std::runtime_error("target_estimation_amd: the pose stream is an output of dense launches");
  if (p.q_delta && (p.idx || p.n_ticks > 1)) throw std::runtime_error("target_estimation_amd: the fused query needs a dense single-tick launch");
  if (p.n_ticks > 1 && p.idx) throw std::runtime_error("target_estimation_amd: fused multi-tick launches are dense only");
  if (p.rec_out && (p.idx || p.n_ticks > 1 || p.q_delta))
    throw std::runtime_error("target_estimation_amd: A -> B ticks are dense single-tick launches without the fused query");
  if (p.cls && p.q_delta)
    throw std::runtime_error("target_estimation_amd: a batch with several (Q, R) classes has no fused sphere query (step, then target_batch_intersect_sphere_dev)");
  // The separable kernels of one-class batches write both output streams themselves (kPose; kInnov, with a pose stream in the
  // same tick the pose writer follows it).  Every other kernel -- the dense ones, several (Q, R) classes -- steps as without the
  // streams: one innovation-writer launch on the records BEFORE the step, one pose-writer launch behind every tick.
  const bool streams_in_kernel = t.sep && !p.cls;
  plan.innov_writer_first = p.nis && (!streams_in_kernel || (plan.gated && (t.gate_by_writer || requested_gate_by_writer(p))));
  plan.pose_writer_after_each_tick = p.pose && (!streams_in_kernel || p.nis);
  // A fused request is served tick by tick -- same results, one launch per tick -- where its kernel does not exist: several
  // (Q, R) classes, poses without a kFused | kPose kernel, the dense kernels that would spill.
  plan.tick_by_tick = p.n_ticks > 1 && (p.cls || t.fused_spills || (p.pose && (!streams_in_kernel || t.fused_pose_tick_by_tick)));
  // A schedule: the kFused loop with the table (one tick included), or tick by tick where that kernel does not exist -- the dense
  // layouts, several (Q, R) classes, a pose stream in the same call, StepTraits::fused_dt_tick_by_tick.
  if (requested_dt_sched(p)) {
    plan.tick_by_tick = !t.sep || p.cls || p.pose || t.fused_dt_tick_by_tick;
    plan.dt_table = !plan.tick_by_tick;
    check_dt_sched(p, plan.dt_table);
  }
  plan.variant = (requested_variant(p) | (plan.dt_table ? (unsigned)kFused : 0u)) & ~((plan.tick_by_tick ? kFused : 0u) | (plan.pose_writer_after_each_tick ? kPose : 0u) |
                                          (plan.innov_writer_first ? kInnov : 0u));
  if (!variant_shipped(plan.variant, t)) throw std::runtime_error("target_estimation_amd: no step kernel for this request");
  return plan;
}

}  // namespace te
