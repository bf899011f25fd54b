// kf_population.hpp -- the tick of a whole manager (one batch per motion model) as ONE launch: host side of
// kf_step_population_kernel (kf_step_sep.hpp).  Reference semantics served: every target of every model advances each
// tick (src/target_manager.cpp:190-225); the models' filters are independent, so their order inside the tick is free.
#pragma once
#include <hip/hip_runtime.h>

#include "kf_ops.hpp"

namespace te {

// parts[k] = the dense single-tick launch parameters of the batch of model type k (ModelType order), n == 0 for an absent
// model.  Every present batch: axis-separable layout with packed groups, one (Q, R) class, no slot list, one tick, the same
// precision `dtype`.  query: the fused own-time sphere query (q_delta set in every present part).  ab: A -> B tick (rec_out set
// in every present part; not together with the query).  reverse: walk the whole population last to first (zig-zag).
// A part with StepParams::pose set also writes the tick's poses (one block, pose_ring / pose_tick_stride unused); other parts may
// have none.
// A part with StepParams::nis set also writes the tick's innovation stream; then the launch is a plain tick in place: no query, no
// A -> B, no pose in any part (the caller adds the query and the poses as launches of their own).
// shared: every present batch is in the shared-axes storage form (te_layout.hpp; fp64 only) instead of the plain one.
void launch_population_step(int dtype, const StepParams parts[4], bool query, bool ab, bool reverse, hipStream_t s, bool shared = false);

// A temporally fused replay of the whole population as ONE launch (kf_step_sep.hpp, kf_step_population_fused_kernel).  parts[k] = the
// dense fused launch parameters of the batch of model type k, as Batch::step_fused_gated hands them to its own launch: n_ticks >= 1
// (the same in every present part), in place, the plain form, no pose stream.  gated: the gated loop -- every present part has
// StepParams::fused_gate set with its NIS rows (fused_gate_nis_max 0: that part's plain stream; fused_gate_k -1: no policy) -- else
// the plain loop, no part with fused_gate.  dt_tab: the call's time-step table in device memory [n_ticks] (every present part has
// StepParams::dt_sched set), or null.  The grid is split as launch_population_step's and never reversed.  Throws for anything else,
// and for an instantiation that is not shipped (step_variant.hpp, population_fused_ok).
void launch_population_fused(int dtype, const StepParams parts[4], bool gated, const double* dt_tab, hipStream_t s);

}  // namespace te
