// te_clock.hpp -- the compensated (two-double) clock behind every target's time.
//
// A target's time is t_base[slot] + t_acc: the batch clock t_acc advances on batch-wide ticks, the per-slot offset t_base
// on by-id updates (and is t0 - t_acc at init).  With single doubles both terms carry rounding errors of the size of
// ulp(batch clock): a target created at t0 = 0 after the batch clock has reached a day is off by ulp(86400) per by-id
// update, far more than the reference's own t_ = t_ + dt drifts (target_interface.cpp:151).  As hi + lo pairs, advanced
// by TwoSum (and TwoProd for dt * n_ticks), both terms are exact to about 2^-106 of their size, and the time read back is
// rounded once: its error is that of the target's own time, whatever the batch clock is.
//
// Included by host code, by the kernels and by the g++ host tests (which define __host__ / __device__ away).
#pragma once

// Every operation below relies on the rounding of each sum: no contraction into FMAs (hipcc's default is contract = fast).
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace te {

struct alignas(16) TClock {
  double hi, lo;   // value = hi + lo, |lo| <= ulp(hi) / 2 after every operation below
};

// s + e == a + b exactly (Knuth's TwoSum; no ordering of |a|, |b| needed)
__host__ __device__ inline void te_two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// (hi, lo) of a + b with hi = round(a + b)
__host__ __device__ inline TClock te_renorm(double a, double b) {
  TClock r;
  te_two_sum(a, b, r.hi, r.lo);
  return r;
}

// c + d, then d2 (the low part of d, or 0)
__host__ __device__ inline TClock te_clock_add(TClock c, double d, double d2 = 0.0) {
  double s, e;
  te_two_sum(c.hi, d, s, e);
  return te_renorm(s, e + (c.lo + d2));
}

// c + dt * n: the product is split exactly (TwoProd with an FMA) before it is added
__host__ __device__ inline TClock te_clock_add_ticks(TClock c, double dt, double n) {
  const double p = dt * n;
  return te_clock_add(c, p, __builtin_fma(dt, n, -p));
}

// a - b as a pair (the offset of a new target from the batch clock)
__host__ __device__ inline TClock te_clock_sub(double a, TClock b) {
  double s, e;
  te_two_sum(a, -b.hi, s, e);
  return te_renorm(s, e - b.lo);
}

// the time b + a, rounded once (up to the 2^-106-relative terms)
__host__ __device__ inline double te_clock_time(TClock b, TClock a) {
  double s, e;
  te_two_sum(b.hi, a.hi, s, e);
  return s + (e + (b.lo + a.lo));
}

// t1 - (b + a): the query offset of getEstimated*(t1) from the unrounded time (t1 - s is exact when t1 is near the time)
__host__ __device__ inline double te_clock_offset(double t1, TClock b, TClock a) {
  double s, e;
  te_two_sum(b.hi, a.hi, s, e);
  return (t1 - s) - (e + (b.lo + a.lo));
}

}  // namespace te

#ifdef __clang__
#pragma clang fp contract(fast)   // back to hipcc's default for what follows
#endif
