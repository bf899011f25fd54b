// kf_ops_impl.hpp -- builds the Ops table entry of one (model, precision, G); included only by
// the kf_model_*.hip translation units.
#pragma once
#include "kf_ops.hpp"
#include "kf_step.hpp"
#include "kf_step_sep.hpp"

#include <algorithm>
#include <cstdlib>
#include <iterator>
#include <stdexcept>
#include <utility>

namespace te {

// host-side launch parameters -> the kernels' argument block
template <typename T>
inline StepArgs<T> make_step_args(const StepParams& p) {
  StepArgs<T> a;
  a.rec = p.rec; a.rec_out = p.rec_out; a.qr = static_cast<const T*>(p.qr); a.cls = p.cls; a.n = p.n; a.idx = p.idx;
  a.meas = static_cast<const T*>(p.meas); a.meas_ld = p.meas_ld; a.has_meas = p.has_meas;
  a.dt_per = p.dt_per; a.dt = p.dt; a.t_base = p.t_base; a.nm_base = p.nm_base;
  a.n_ticks = p.n_ticks; a.tick_stride = p.tick_stride; a.has_stride = p.has_stride;
  a.q_origin[0] = p.q_origin[0]; a.q_origin[1] = p.q_origin[1]; a.q_origin[2] = p.q_origin[2];
  a.q_radius = p.q_radius; a.q_delta = p.q_delta; a.q_pose = p.q_pose;
  a.reverse = p.reverse; a.nt_meas = p.nt_meas;
  a.o_pose = p.o_pose; a.o_twist = p.o_twist; a.o_acc = p.o_acc; a.done_flag = p.done_flag; a.done_seq = p.done_seq; a.done_count = p.done_count;
  a.live_posted = p.live_posted; a.live_mirror = p.live_mirror; a.live_progress = p.live_progress; a.live_done = p.live_done;
  a.live_ring = p.live_ring; a.live_first = p.live_first;
  a.live_spin_limit = p.live_spin_limit; a.live_idle_ticks = p.live_idle_ticks; a.live_flags = p.live_flags; a.live_pose = p.live_pose; a.live_pose_ld = p.live_pose_ld;
  a.pose = p.pose; a.pose_ld = p.pose_ld; a.pose_tick_stride = p.pose_tick_stride; a.pose_ring = p.pose_ring;
  a.tile_blk = p.tile_blk; a.tile_uni = p.tile_uni; a.promote = p.promote;
  a.nis = p.nis; a.innov = p.innov; a.innov_ld = p.innov_ld;
  return a;
}

// The INNOV step kernels (kf_step_sep.hpp; dense single ticks of the separable layouts) are instantiated in translation units of
// their own, kf_innov_{uv,ua,ar,av}.hip (kf_innov_impl.hpp), so that the build stays parallel and the kf_model_* / kf_shared_*
// objects hold the instantiations they always held; OpsImpl::step reaches them through this declaration.
template <class M, typename T, int LAYOUT>
void launch_sep_innov_step(const StepArgs<T>& a, unsigned blocks, unsigned threads, hipStream_t s);

// The gated kInnov kernels (kf_step_sep.hpp, kf_step_sep_gate_kernel), in kf_gate_{uv,ua,ar,av}.hip (kf_gate_impl.hpp) likewise.
template <class M, typename T, int LAYOUT>
void launch_sep_gate_step(const StepArgs<T>& a, double gate, unsigned blocks, unsigned threads, hipStream_t s);

// The gated by-id kernels (kf_step_sep.hpp, kf_step_sep_gate_indexed_kernel), in kf_gate_id_{uv,ua,ar,av}.hip (kf_gate_id_impl.hpp) likewise.
template <class M, typename T, int LAYOUT>
void launch_sep_gate_id_step(const StepArgs<T>& a, const GateById& g, unsigned blocks, unsigned threads, hipStream_t s);

// The gated resident kernels (kf_step_sep.hpp, kf_step_sep_live_gate_kernel), in kf_live_gate_{uv,ua,ar,av}.hip
// (kf_live_gate_impl.hpp) likewise; live_gate_blocks_per_cu is the occupancy query about them, made where they are instantiated.
template <class M, typename T, int LAYOUT>
void launch_sep_live_gate_step(const StepArgs<T>& a, const LiveGate& g, unsigned blocks, unsigned threads, hipStream_t s);
template <class M, typename T, int LAYOUT>
int live_gate_blocks_per_cu();

// The launched fused gated kernels (kf_step_sep.hpp, kf_step_sep_fused_gate_kernel), in kf_fused_gate_{uv,ua,ar,av}.hip
// (kf_fused_gate_impl.hpp) likewise.
template <class M, typename T, int LAYOUT>
void launch_sep_fused_gate_step(const StepArgs<T>& a, const FusedGate& g, unsigned blocks, unsigned threads, hipStream_t s);

// The launched fused kernels with a time-step table (kf_step_sep.hpp, kf_step_sep_fused_dt_kernel / kf_step_sep_fused_gate_dt_kernel), in
// kf_fused_dt_{uv,ua,ar,av}.hip (kf_fused_dt_impl.hpp) likewise.
template <class M, typename T, int LAYOUT>
void launch_sep_fused_dt_step(const StepArgs<T>& a, const double* dt_tab, unsigned blocks, unsigned threads, hipStream_t s);
template <class M, typename T, int LAYOUT>
void launch_sep_fused_gate_dt_step(const StepArgs<T>& a, const FusedGate& g, const double* dt_tab, unsigned blocks, unsigned threads, hipStream_t s);

// reacquire_kernel (kf_reacquire_impl.hpp), in kf_reacquire_{uv,ua,ar,av}.hip likewise: one instance per OpsImpl.
template <class M, typename T, int G, int LAYOUT>
void launch_reacquire(const ReacquireArgs& a, hipStream_t s);

template <class M, typename T, int G, int LAYOUT = LAYOUT_FULL>
struct OpsImpl {
  using C = Cfg<M, T, G, LAYOUT>;

  static constexpr bool kHasLive = LAYOUT == LAYOUT_SEPARABLE_PACKED;
  // with_outputs: 1 = the variant with the per-tick query / pose output (kLive2), 2 = the gated one (kf_step_sep_live_gate_kernel)
  static long live_capacity(int with_outputs) {
    if constexpr (kHasLive) {
      int per_cu = 0, dev = 0;
      hipDeviceProp_t prop;
      if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
      if (with_outputs == 2) {
        per_cu = live_gate_blocks_per_cu<M, T, LAYOUT>();
        if (per_cu <= 0) return 0;
      } else {
        const void* kernel = with_outputs ? (const void*)kf_step_sep_kernel<M, T, LAYOUT, kFused | kLive2>
                                          : (const void*)kf_step_sep_kernel<M, T, LAYOUT, kFused | kLive1>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess) return 0;
      }
      // Measured on an MI355X with the relay's start word (tools/live_capacity.py --probe, profiles/r03_live_capacity.txt): the
      // largest grid that becomes resident is the query's figure for every kernel at up to 6 wavefronts per SIMD, but 28 per CU
      // where the query says 32 (8 per SIMD).  And a device that full starves everybody else: with 22 or more resident
      // wavefronts per CU (of 24 / 28) a device-to-device copy on another stream -- the caller's ring refill -- waited for the
      // session to end, with 18.4 of 20 it took its usual 0.4 ms.  So: at most 5 per SIMD, and one block per CU in hand.
      if (per_cu > 20) per_cu = 20;
      return (long)(per_cu > 1 ? per_cu - 1 : 1) * (long)prop.multiProcessorCount;
    } else {
      return 0;
    }
  }
  // The temporally fused POSE kernels that would cost a wavefront per SIMD or spill (profiles/r05_pose_kernel_resources.txt):
  // angular_rates fp32 on packed groups (97 registers, 4 waves per SIMD against the twin's 91 / 5; held to 5: 12 B of scratch) and
  // uniform_acceleration fp32 on packed groups (66 / 7 against 62 / 8; held to 8: 12 B of scratch).  Not instantiated: a fused
  // request with poses is served tick by tick by the single-tick POSE kernel -- same results, one launch per tick.
  static constexpr bool kFusedPoseTickByTick = sizeof(T) == 4 && LAYOUT == LAYOUT_SEPARABLE_PACKED &&
                                               (M::TYPE == ANGULAR_RATES || M::TYPE == UNIFORM_ACCELERATION);
  // A few temporally fused instantiations of the dense kernel do not fit the register file and would spill hundreds of bytes
  // per lane to scratch (228 / 116 / 340 / 352 B).  Not instantiated: a fused request is served tick by tick -- same results.
  static constexpr bool kFusedSpills = (M::TYPE == ANGULAR_RATES && sizeof(T) == 8 && G == 3 && LAYOUT == LAYOUT_PACKED) ||
                                       (M::TYPE == ANGULAR_VELOCITIES && sizeof(T) == 4 && G == 1 && LAYOUT == LAYOUT_FULL) ||
                                       (M::TYPE == ANGULAR_VELOCITIES && sizeof(T) == 8 && G == 1 && LAYOUT == LAYOUT_PACKED) ||
                                       (M::TYPE == ANGULAR_RATES && sizeof(T) == 8 && G == 6 && LAYOUT == LAYOUT_PACKED);
  // Gated separable instantiations that would spill or need scratch are not shipped: their gate is the innovation writer's mask
  // row and the plain step (profiles/r11_gate_kernel_resources.txt).  None does.
  static constexpr bool kGateByWriter = false;
  // Launched fused gated instantiations that would need scratch are not shipped: such a batch's fused gated call is served tick
  // by tick (profiles/fused_gate_kernel_resources.txt).  None does.
  static constexpr bool kFusedGateTickByTick = false;
  static constexpr bool kHasFusedGate = C::SEP && !C::SHARED && !kGateByWriter && !kFusedGateTickByTick;
  // Launched fused instantiations with a time-step table that would need scratch are not shipped: such a batch's schedule call is
  // served tick by tick (profiles/dt_schedule_kernel_resources.txt).  None does.
  static constexpr bool kFusedDtTickByTick = false;
  static constexpr bool kFusedGateDtTickByTick = false;
  static constexpr bool kHasFusedDt = C::SEP && !C::SHARED && !kFusedDtTickByTick;
  static constexpr bool kHasFusedGateDt = kHasFusedGate && !kFusedGateDtTickByTick;
  static constexpr StepTraits kTraits{C::SEP, C::SHARED, C::UT, kHasLive, kFusedPoseTickByTick, kFusedSpills, C::TPW, kGateByWriter, kFusedGateTickByTick,
                                      kFusedDtTickByTick, kFusedGateDtTickByTick};
  // the pose-writer launch behind a tick whose kernel has no pose output: outputs_kernel into the tick's block
  static void write_pose_block(const StepParams& p, double* pose, hipStream_t s) {
    OutArgs o;
    o.rec = p.rec_out ? p.rec_out : p.rec;   // (an A -> B tick has written the new records there)
    o.idx = nullptr; o.n = p.n; o.pose = nullptr; o.twist = nullptr; o.acc = nullptr;
    o.at_time = 0; o.t1 = 0.0; o.t_acc = TClock{0.0, 0.0}; o.t_base = p.t_base;
    o.pose_soa = pose; o.pose_ld = p.pose_ld;
    outputs(o, s);
  }
  // One launch of the step kernel of variant V.  A variant this OpsImpl does not ship (variant_shipped) is not instantiated; the
  // kInnov kernels live in translation units of their own (launch_sep_innov_step above).
  template <unsigned V>
  static bool launch_if(unsigned v, const StepArgs<T>& a, unsigned blocks, unsigned threads, hipStream_t s) {
    if constexpr (variant_shipped(V, kTraits)) {
      if (v != V) return false;
      if constexpr (V == kInnov) launch_sep_innov_step<M, T, LAYOUT>(a, blocks, threads, s);
      else if constexpr (C::SEP) hipLaunchKernelGGL((kf_step_sep_kernel<M, T, LAYOUT, V>), dim3(blocks), dim3(threads), 0, s, a);
      else hipLaunchKernelGGL((kf_step_kernel<M, T, G, LAYOUT, V>), dim3(blocks), dim3(threads), 0, s, a);
      return true;
    } else {
      return false;
    }
  }
  template <const auto& LIST, size_t... I>
  static void launch_variant(std::index_sequence<I...>, unsigned v, const StepArgs<T>& a, unsigned blocks, unsigned threads, hipStream_t s) {
    if (!(launch_if<LIST[I]>(v, a, blocks, threads, s) || ...)) throw std::runtime_error("target_estimation_amd: no step kernel for this request");
  }
  static void launch_variant(unsigned v, const StepArgs<T>& a, unsigned blocks, unsigned threads, hipStream_t s) {
    if constexpr (C::SEP) launch_variant<kSepVariants>(std::make_index_sequence<std::size(kSepVariants)>{}, v, a, blocks, threads, s);
    else launch_variant<kDenseVariants>(std::make_index_sequence<std::size(kDenseVariants)>{}, v, a, blocks, threads, s);
  }
  static void launch_gate(const StepArgs<T>& a, double gate, unsigned blocks, unsigned threads, hipStream_t s) {
    if constexpr (C::SEP && !kGateByWriter) launch_sep_gate_step<M, T, LAYOUT>(a, gate, blocks, threads, s);
    else throw std::runtime_error("target_estimation_amd: no gated step kernel for this request");
  }
  static void launch_gate_by_id(const StepArgs<T>& a, const StepParams& p, unsigned blocks, unsigned threads, hipStream_t s) {
    if constexpr (C::SEP && !kGateByWriter) {
      GateById g;
      g.gate = p.gate; g.k = p.gate_id_k; g.run = p.reacq_run; g.p0_tab = p.reacq_p0; g.p0_idx = p.reacq_p0_idx; g.event = p.gate_id_event;
      launch_sep_gate_id_step<M, T, LAYOUT>(a, g, blocks, threads, s);
    } else {
      throw std::runtime_error("target_estimation_amd: the update gate by id: no gated indexed kernel for this batch");
    }
  }
  static void launch_live_gate(const StepArgs<T>& a, const StepParams& p, unsigned blocks, unsigned threads, hipStream_t s) {
    if constexpr (kHasLive) {
      LiveGate g;
      g.gate = p.live_gate_nis_max; g.nis = p.live_gate_nis; g.nis_stride = p.live_gate_nis_stride; g.nis_ring = p.live_gate_nis_ring;
      g.k = p.live_gate_k; g.run = p.reacq_run; g.p0_tab = p.reacq_p0; g.p0_idx = p.reacq_p0_idx;
      g.event = p.live_gate_event; g.event_stride = p.live_gate_event_stride; g.event_ring = p.live_gate_event_ring;
      launch_sep_live_gate_step<M, T, LAYOUT>(a, g, blocks, threads, s);
    } else {
      throw std::runtime_error("target_estimation_amd: the resident gate: no resident kernel for this batch");
    }
  }
  static void launch_fused_dt(const StepArgs<T>& a, const StepParams& p, unsigned blocks, unsigned threads, hipStream_t s) {
    if constexpr (kHasFusedDt) launch_sep_fused_dt_step<M, T, LAYOUT>(a, p.dt_tab, blocks, threads, s);
    else throw std::runtime_error("target_estimation_amd: the time-step schedule: no fused kernel with a table for this batch");
  }
  static void launch_fused_gate(const StepArgs<T>& a, const StepParams& p, unsigned blocks, unsigned threads, hipStream_t s, bool dt_table = false) {
    if constexpr (kHasFusedGate) {
      FusedGate g;
      g.gate = p.fused_gate_nis_max; g.nis = p.fused_gate_nis; g.nis_stride = p.fused_gate_nis_stride; g.nis_ring = p.fused_gate_nis_ring;
      g.innov = p.fused_gate_innov; g.innov_ld = p.fused_gate_innov_ld; g.innov_stride = p.fused_gate_innov_stride;
      g.k = p.fused_gate_k; g.run = p.reacq_run; g.p0_tab = p.reacq_p0; g.p0_idx = p.reacq_p0_idx;
      // (a predict-only call changes no run and, like the single ticks, writes no event row)
      g.event = p.meas ? p.fused_gate_event : nullptr; g.event_stride = p.fused_gate_event_stride; g.event_ring = p.fused_gate_event_ring;
      if (dt_table) {
        if constexpr (kHasFusedGateDt) launch_sep_fused_gate_dt_step<M, T, LAYOUT>(a, g, p.dt_tab, blocks, threads, s);
        else throw std::runtime_error("target_estimation_amd: the time-step schedule: no fused gated kernel with a table for this batch");
      } else {
        launch_sep_fused_gate_step<M, T, LAYOUT>(a, g, blocks, threads, s);
      }
    } else {
      throw std::runtime_error("target_estimation_amd: the fused gate: no fused gated kernel for this batch");
    }
  }
  // A fused gated request without a kernel of its own: tick s of the call as the single gated request target_batch_step_sequence_reacquire
  // makes for it, planned and launched on its own.
  static void step_fused_gate_tick_by_tick(const StepParams& p, hipStream_t s) {
    for (long t = 0; t < (long)p.n_ticks; ++t) {
      StepParams q = p;
      q.fused_gate = 0; q.n_ticks = 1; q.tick_stride = 0; q.has_stride = 0;
      if (p.dt_sched) { q.dt = p.dt_host[t]; q.dt_sched = 0; q.dt_host = nullptr; q.dt_tab = nullptr; }   // (a single tick takes its dt by value)
      q.meas = p.meas ? static_cast<const char*>(p.meas) + (size_t)t * (size_t)p.tick_stride * sizeof(T) : nullptr;
      q.has_meas = p.has_meas ? p.has_meas + t * p.has_stride : nullptr;
      const long b = p.fused_gate_nis_ring > 0 ? t % p.fused_gate_nis_ring : t;
      q.nis = p.fused_gate_nis + b * p.fused_gate_nis_stride;
      q.innov = p.fused_gate_innov ? p.fused_gate_innov + b * p.fused_gate_innov_stride : nullptr; q.innov_ld = p.fused_gate_innov_ld;
      q.gate = p.fused_gate_nis_max;
      if (p.fused_gate_k >= 0) {
        q.reacq = 1; q.reacq_k = p.fused_gate_k;
        q.reacq_event = p.fused_gate_event ? p.fused_gate_event + (p.fused_gate_event_ring > 0 ? t % p.fused_gate_event_ring : t) * p.fused_gate_event_stride : nullptr;
      }
      if (p.pose) { q.pose = p.pose + (p.pose_ring > 0 ? t % p.pose_ring : t) * p.pose_tick_stride; q.pose_tick_stride = 0; q.pose_ring = 0; }
      step(q, s);
    }
  }
  // The launches of a request are plan_step's (step_variant.hpp): [innovation writer,] then once, or once per tick, the step
  // kernel [and the pose writer].
  static void step(const StepParams& p, hipStream_t s) {
    if (p.n <= 0) return;
    const StepPlan plan = plan_step(kTraits, p);
    const long waves = (p.n + C::TPW - 1) / C::TPW;
    if (plan.fused_gated && plan.tick_by_tick) { step_fused_gate_tick_by_tick(p, s); return; }
    if (sv_live(plan.variant)) {   // resident launch: one wavefront per workgroup, every workgroup resident (Batch::live_start checked the capacity)
      // + 1: the relay wavefront (kf_step.hpp live_relay)
      if (plan.live_gated) launch_live_gate(make_step_args<T>(p), p, (unsigned)waves + 1, 64, s);
      else launch_variant(plan.variant, make_step_args<T>(p), (unsigned)waves + 1, 64, s);
      return;
    }
    StepParams q = p;
    if (plan.innov_writer_first) {
      InnovArgs w;
      w.rec = p.rec; w.qr = p.qr; w.cls = p.cls; w.n = p.n; w.meas = p.meas; w.meas_ld = p.meas_ld; w.has_meas = p.has_meas; w.dt = p.dt;
      w.tile_blk = p.tile_blk; w.tile_uni = p.tile_uni; w.nis = p.nis; w.innov = p.innov; w.innov_ld = p.innov_ld;
      if (plan.gated) {   // the writer decides: its mask row is the step's has_meas
        if (!p.gate_row) throw std::runtime_error("target_estimation_amd: a gated tick of this layout needs the batch's mask row");
        innov_gate(w, p.gate, p.gate_row, s);
        q.has_meas = p.gate_row; q.has_stride = 0;
      } else {
        innov(w, s);
      }
      q.nis = nullptr; q.innov = nullptr;
    }
    const bool gate_kernel = plan.gated && !plan.innov_writer_first;
    static const int nt_env = [] { const char* e = std::getenv("TE_NT_MEAS"); return e ? std::atoi(e) : -1; }();
    if (nt_env >= 0) q.nt_meas = nt_env;
    static const long small_grid = [] { const char* e = std::getenv("TE_SMALL_GRID_WAVES"); return e ? std::atol(e) : 1024L; }();
    // small (latency-bound) grids: one wavefront per workgroup spreads the waves over more CUs
    const int wpb = waves <= small_grid ? 1 : C::SEP ? 4 : C::WPB;
    const unsigned blocks = (unsigned)((waves + wpb - 1) / wpb);
    if (plan.tick_by_tick) {
      q.n_ticks = 1;
      if (p.pose) { q.pose_tick_stride = 0; q.pose_ring = 0; }
    }
    if (p.dt_sched && !plan.dt_table) { q.dt_sched = 0; q.dt_host = nullptr; q.dt_tab = nullptr; }   // (single ticks take their dt by value)
    for (int t = 0, launches = plan.tick_by_tick ? p.n_ticks : 1; t < launches; ++t) {
      double* pose = p.pose;
      if (plan.tick_by_tick) {   // tick t's measurement block, mask row and pose block
        q.meas = p.meas ? static_cast<const char*>(p.meas) + (size_t)t * (size_t)p.tick_stride * sizeof(T) : nullptr;
        q.has_meas = p.has_meas ? p.has_meas + (long)t * p.has_stride : nullptr;
        if (p.dt_sched) q.dt = p.dt_host[t];
        if (p.pose) pose = p.pose + (p.pose_ring > 0 ? (long)t % p.pose_ring : (long)t) * p.pose_tick_stride;
      }
      q.pose = plan.pose_writer_after_each_tick ? nullptr : pose;
      if (plan.gate_by_id) launch_gate_by_id(make_step_args<T>(q), p, blocks, 64u * (unsigned)wpb, s);
      else if (plan.fused_gated) launch_fused_gate(make_step_args<T>(q), p, blocks, 64u * (unsigned)wpb, s, plan.dt_table);
      else if (plan.dt_table) launch_fused_dt(make_step_args<T>(q), p, blocks, 64u * (unsigned)wpb, s);
      else if (gate_kernel) launch_gate(make_step_args<T>(q), p.gate, blocks, 64u * (unsigned)wpb, s);
      else launch_variant(plan.variant, make_step_args<T>(q), blocks, 64u * (unsigned)wpb, s);
      if (plan.reacquire_after_step) reacquire(make_reacquire_args(p), s);   // (p: the caller's mask and NIS row; gated ticks are single)
      if (plan.pose_writer_after_each_tick) write_pose_block(q, pose, s);
    }
  }
  static void init(const InitArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL((init_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + 127) / 128)), dim3(128), 0, s, a);
  }
  static void get_state(char* rec, const int* idx, long n, double* x, double* P, const double* tile_blk, const int* tile_uni, hipStream_t s) {
    if (n <= 0) return;
    const long th = n * C::N;
    hipLaunchKernelGGL((get_state_kernel<M, T, G, LAYOUT>), dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s, rec, idx, n, x, P, tile_blk, tile_uni);
  }
  static void settle(char* rec, long n, const double* tile_blk, const int* tile_uni, hipStream_t s) {
    if constexpr (C::UT) {
      if (n <= 0) return;
      hipLaunchKernelGGL((settle_tiles_kernel<M, T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rec, n, tile_blk, tile_uni);
    }
  }
  static void set_state(char* rec, const int* idx, long n, const double* x, const double* P, const double* uw, hipStream_t s) {
    if (n <= 0) return;
    const long th = n * C::N;
    hipLaunchKernelGGL((set_state_kernel<M, T, G, LAYOUT>), dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s, rec, idx, n, x, P, uw);
  }
  static void move_records(char* rec, const int* src, const int* dst, long m, TClock* t_base, int* nm_base, int* cls, hipStream_t s) {
    const int th = C::G * C::RW;
    for (long done = 0; done < m; done += 65535) {   // grid.y limit
      const long part = std::min<long>(65535, m - done);
      hipLaunchKernelGGL((move_records_kernel<M, T, G, LAYOUT>), dim3((th + 255) / 256, (unsigned)part), dim3(256), 0, s, rec, src + done,
                         dst + done, part, t_base, nm_base, cls);
    }
  }
  static void move_record(char* rec, long src, long dst, TClock* t_base, int* nm_base, int* cls, hipStream_t s) {
    const int th = C::G * C::RW;
    hipLaunchKernelGGL((move_record_kernel<M, T, G, LAYOUT>), dim3((th + 255) / 256), dim3(256), 0, s, rec, src, dst, t_base, nm_base, cls);
  }
  static void outputs(const OutArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL((outputs_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + kOutputsBlock - 1) / kOutputsBlock)), dim3(kOutputsBlock), 0, s, a);
  }
  static void innov(const InnovArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL((innov_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + 127) / 128)), dim3(128), 0, s, a);
  }
  static void innov_gate(const InnovArgs& a, double gate, unsigned char* has_eff, hipStream_t s) {
    if (a.n <= 0) return;
    innov(a, s);
    hipLaunchKernelGGL((gate_mask_kernel<>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, (const double*)a.nis, a.has_meas, a.meas != nullptr ? 1 : 0,
                       a.n, gate, has_eff);
  }
  static void reacquire(const ReacquireArgs& a, hipStream_t s) {
    if (a.n <= 0 || !a.meas) return;
    launch_reacquire<M, T, G, LAYOUT>(a, s);
  }
  static void outputs_rows(const OutArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL((outputs_rows_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + kOutputsBlock - 1) / kOutputsBlock)), dim3(kOutputsBlock), 0, s, a);
  }
  static void pack_meas(const double* aos, long n, void* soa, long ld, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((pack_meas_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, aos, n, static_cast<T*>(soa), ld);
  }
  static void intersect(const IntersectArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL((intersect_kernel<M, T, G, LAYOUT>), dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
  }
  static void expand(char* rec, char* rec_plain, long n, hipStream_t s) {
    if constexpr (C::SHARED) {
      if (n <= 0) return;
      hipLaunchKernelGGL((expand_shared_kernel<M, T>), dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, rec, rec_plain, n);
    }
  }
  static const Ops* get() {
    // (host code sees the shared-axes form as layout 3 with the flag set: te_layout.hpp)
    static const Ops ops = {
        LayoutInfo{C::N, C::K, G, C::SHARED ? (int)LAYOUT_SEPARABLE_PACKED : LAYOUT, C::TPW, C::LPT, C::RW, C::TILE_BYTES, C::TILE_PAYLOAD, C::SHARED ? 1 : 0,
                   C::UT ? C::LW : 0, C::UT ? C::LIN_CHUNKS : 0},
        C::WPB, &step, &live_capacity, &init, &get_state, &set_state, &move_record, &move_records, &outputs, &pack_meas, &intersect, &outputs_rows, &innov, &innov_gate,
        C::SHARED ? &expand : nullptr, C::UT ? &settle : nullptr, &reacquire, kHasFusedGate ? 1 : 0, kHasFusedDt ? 1 : 0, kHasFusedGateDt ? 1 : 0};
    return &ops;
  }
};

}  // namespace te
