// dt_schedule.hpp -- the time-step schedule of a multi-tick call: a host array dt[n], tick s of the call runs with dt[s]
// (target_batch_step_sequence_dt / _step_fused_dt / target_manager_step_sequence_all_dt).  Plain C++17 without a HIP dependency
// (tests/host/dt_schedule_test.cpp compiles it with g++): the view handed to Batch / Shard / TargetManager, the clock accounting
// of a call, and the key a recorded graph is filed under.
//
// A default-constructed schedule is "none": the call runs with its one scalar dt, as it always did.
#pragma once
#include <cstring>
#include <vector>

#ifndef __host__
#define __host__
#define __device__
#define TE_DT_SCHEDULE_DEFINED_HD_
#endif
#include "te_clock.hpp"
#ifdef TE_DT_SCHEDULE_DEFINED_HD_
#undef __host__
#undef __device__
#undef TE_DT_SCHEDULE_DEFINED_HD_
#endif

namespace te {

// The most ticks ONE launch serves from a device table: the kernels address entry s at a 32-bit byte offset 8 s (kf_step_sep.hpp,
// DTTAB).  A longer call runs its ticks as single launches -- same results.
constexpr long kDtTabMaxTicks = 1L << 28;

struct DtSchedule {
  const double* dt = nullptr;   // host array [n], read before the call that takes it returns; null: no schedule
  long n = 0;

  DtSchedule() = default;
  DtSchedule(const double* dt_host, long n_ticks) : dt(dt_host), n(dt_host ? n_ticks : 0) {}

  bool on() const { return dt != nullptr; }
  // the dt of tick s: the schedule's entry, or the call's scalar
  double at(long s, double scalar) const { return dt ? dt[s] : scalar; }
  // ticks [first, first + count) as a schedule of their own (a call served in parts)
  DtSchedule part(long first, long count) const { return dt ? DtSchedule(dt + first, count) : DtSchedule(); }

  // The batch clock behind the call's ticks: one te_clock_add per tick, in order -- what n single ticks (Batch::step_dense)
  // leave, bit for bit.  Never dt * n: the entries differ, and even where they do not the single ticks' sum is the contract.
  TClock advance(TClock c) const {
    for (long s = 0; s < n; ++s) c = te_clock_add(c, dt[s]);
    return c;
  }

  // The key of a recorded graph: the schedule's values AS BITS (a recording bakes every tick's dt into its launch), so 0.0 and
  // -0.0 differ and a NaN equals itself.  A scalar call's key is empty; a schedule never matches it.
  std::vector<double> key() const { return dt ? std::vector<double>(dt, dt + n) : std::vector<double>(); }
  bool same_bits(const std::vector<double>& k) const {
    if (!dt) return false;
    return (long)k.size() == n && (n == 0 || std::memcmp(k.data(), dt, (size_t)n * sizeof(double)) == 0);
  }
};

// Does a recording filed under (key, scalar) serve a call with (sched, dt)?  A recording of a scalar call serves scalar calls with
// the same dt; a recording of a schedule serves calls whose schedule has the same bits.
inline bool dt_key_matches(const std::vector<double>& key, bool key_is_schedule, double key_scalar, const DtSchedule& sched, double dt) {
  if (key_is_schedule != sched.on()) return false;
  return key_is_schedule ? sched.same_bits(key) : key_scalar == dt;
}

// What a recording is filed under: the call's scalar dt, or its schedule's bits.
struct DtKey {
  double dt = 0.0;
  bool is_schedule = false;
  std::vector<double> bits;
  DtKey() = default;
  DtKey(const DtSchedule& sched, double scalar) : dt(scalar), is_schedule(sched.on()), bits(sched.key()) {}
  bool matches(const DtSchedule& sched, double scalar) const { return dt_key_matches(bits, is_schedule, dt, sched, scalar); }
};

}  // namespace te
