// associate_grid_plan.hpp -- no HIP: everything about the GRID form of the association (target_batch_c.h,
// target_batch_associate_grid*) that is not a kernel -- the box rule, the cell map, the narrow / wide classes, the
// bucket hash and the bucket-count plan, the keyed pick, the argument checks.  associate_grid.hip (the kernels), Batch / Shard /
// TargetManager (the host side) and tests/host/associate_grid_plan_host_test.cpp (g++ alone) all build this header.  The table
// row, S^-1, d^2 and the rounds are associate_plan.hpp's, unchanged.
#pragma once
#include <cfloat>
#include <cmath>

#include "associate_plan.hpp"

namespace te {

constexpr long kAssocGridMaxDetections = 1048576;   // TARGET_ASSOC_GRID_MAX_DETECTIONS
constexpr long kAssocGridMinBuckets = 1024;
constexpr long kAssocGridMaxBuckets = 1L << 30;
constexpr double kAssocGridCoordLimit = 1073741824.0;   // 2^30: cell coordinates are clamped to [-2^30, 2^30]
constexpr int kAssocGridThreads = 256;                  // threads of every grid-form workgroup (the resolve step's too)
constexpr int kAssocGridWideWgs = 1024;                 // the fixed grid of the wide target-major scan: it strides over the wide list

// slot classes
constexpr int kAssocGridNone = 0;     // a NaN row: neither narrow nor wide, never a candidate
constexpr int kAssocGridNarrow = 1;
constexpr int kAssocGridWide = 2;

// THE BOX: reach2_a = (gate * S_aa) * (1 + 2^-10), plain multiplies.  In exact arithmetic nu_a^2 <= d2 * S_aa (Cauchy-Schwarz in
// the W inner product: nu_a = e_a^T nu, e_a^T S e_a = S_aa), so the box contains the gate ellipsoid; the factor 1 + 2^-10 leaves
// the rounding of d2 one part in 10^3 of the gate before a pair inside the gate could fall outside the box.
TE_ASSOC_HD inline double assoc_grid_reach2(double gate, double s_aa) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (gate * s_aa) * (1.0 + 0.0009765625);
}

// THE CANDIDATE RULE of the grid form: d2 <= gate AND nu_a * nu_a <= reach2_a on every axis, nu_a the very double assoc_d2 forms
// (the same subtraction).  A NaN anywhere rejects.  d2 is returned for the pick.
TE_ASSOC_HD inline bool assoc_grid_candidate(const double* zhat, const double* W, const double* reach2, double x, double y, double z,
                                             double gate, double* d2_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nx = x - zhat[0], ny = y - zhat[1], nz = z - zhat[2];
  const double d2 = assoc_d2(zhat, W, x, y, z);
  *d2_out = d2;
  return d2 <= gate && nx * nx <= reach2[0] && ny * ny <= reach2[1] && nz * nz <= reach2[2];
}

// THE CELL COORDINATE of one axis: floor(x / cell) in double, clamped to [-2^30, 2^30] (a clamped monotone map keeps neighbours
// neighbours); a NaN goes to -2^30 -- such a position is never a candidate, so where it is binned does not matter.
TE_ASSOC_HD inline int assoc_grid_coord(double x, double cell) {
  double q = std::floor(x / cell);
  if (!(q >= -kAssocGridCoordLimit)) q = -kAssocGridCoordLimit;
  if (q > kAssocGridCoordLimit) q = kAssocGridCoordLimit;
  return (int)q;
}

// THE NARROW LIMIT: lim2 = (cell * (1 - 2^-20))^2, or -1 (no slot is narrow) where that square is not a normal double.
// A valid slot is NARROW iff reach2_a <= lim2 on all three axes.
//
// CLAIM.  If a slot is narrow, every detection x that passes the box rule on axis a lies within +-1 cell of zhat on that axis:
// |coord(x_a) - coord(zhat_a)| <= 1.
// PROOF (u = 2^-53, all roundings to nearest, monotone).  Let L = fl(cell (1 - 2^-20)) <= cell (1 - 2^-20)(1 + u) and lim2 = fl(L L),
// a normal double.  The box rule gives fl(nu nu) <= reach2 <= fl(L L) with nu = fl(x - zhat).  If |nu| > L (1 + 2u), then
// fl(nu nu) >= nu nu (1 - u) > L L (1 + 2u)^2 (1 - u) > L L (1 + u) >= fl(L L): a contradiction.  Hence |nu| <= L (1 + 2u), and
// |x - zhat| <= |nu| (1 + u) <= cell (1 - 2^-20)(1 + 5u) < cell (1 - 2^-21).  In exact arithmetic therefore
// |x / cell - zhat / cell| < 1 - 2^-21.
//   Both computed quotients at most 2^30 in magnitude: each division rounds by at most 2^30 u = 2^-23, so the computed quotients
// differ by less than 1 - 2^-21 + 2^-22 < 1, and two reals less than 1 apart have floors at most 1 apart.
//   One computed quotient beyond 2^30 (say fl(x / cell) > 2^30, clamped to 2^30), the other not: 2^30 is a double and rounding is
// monotone, so x / cell > 2^30 exactly, zhat / cell > 2^30 - 1, and -- 2^30 - 1 is a double too -- fl(zhat / cell) >= 2^30 - 1:
// one cell from the clamp.  Both beyond on the same side: the same clamped coordinate; on opposite sides: impossible.  The
// negative side mirrors this.  (tests/host/associate_grid_plan_host_test.cpp checks the claim on random and on adversarial
// inputs: borders, one ulp either side, negative coordinates, the clamp, cell 1e-3 .. 1e3.)
TE_ASSOC_HD inline double assoc_grid_narrow_limit2(double cell) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double L = cell * (1.0 - 9.5367431640625e-07);
  const double lim2 = L * L;
  return (lim2 >= DBL_MIN && lim2 <= DBL_MAX) ? lim2 : -1.0;
}
// the class of a slot from its row's zhat[0] (NaN: an invalid row) and reach2
TE_ASSOC_HD inline int assoc_grid_class(double zhat0, const double* reach2, double lim2) {
  if (!(zhat0 == zhat0)) return kAssocGridNone;
  return (reach2[0] <= lim2 && reach2[1] <= lim2 && reach2[2] <= lim2) ? kAssocGridNarrow : kAssocGridWide;
}

// THE BUCKET of a cell among H buckets (H a power of two).  Collisions are harmless: the exact tests filter what a walk meets.
TE_ASSOC_HD inline unsigned assoc_grid_hash(int cx, int cy, int cz, unsigned mask) {
  unsigned h = (unsigned)cx * 0x9E3779B1u ^ (unsigned)cy * 0x85EBCA77u ^ (unsigned)cz * 0xC2B2AE3Du;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 13;
  return h & mask;
}

// THE BUCKET COUNT for at most `count` binned entries: a power of two >= 2 * count and >= 1024; forced > 0 (TE_ASSOC_GRID_BUCKETS)
// sets it regardless, so that small calls live entirely in collisions.
inline long plan_assoc_grid_buckets(long count, long forced) {
  if (forced > 0) return forced;
  long h = kAssocGridMinBuckets;
  while (h < 2 * count && h < kAssocGridMaxBuckets) h <<= 1;
  return h;
}
// TE_ASSOC_GRID_BUCKETS as read from the environment: 0 (null, junk, < 1) = planned, else rounded DOWN to a power of two, at most 2^30
inline long assoc_grid_forced_buckets_from(const char* env) {
  if (!env || !env[0]) return 0;
  char* end = nullptr;
  const long v = std::strtol(env, &end, 10);
  if (end == env || v < 1) return 0;
  long h = 1;
  while (h * 2 <= v && h < kAssocGridMaxBuckets) h <<= 1;
  return h;
}

// THE KEYED PICK: the walks of the grid form are not in ascending index order (bucket order, repeats through collisions), so the
// full key (d2, index) is compared explicitly; visiting the same entry twice changes nothing.
TE_ASSOC_HD inline void assoc_take_keyed(AssocBest& best, double d2, int idx) {
  if (best.idx < 0 || d2 < best.d2 || (d2 == best.d2 && idx < best.idx)) { best.d2 = d2; best.idx = idx; }
}

// THE REFUSALS of the grid form: check_assoc_args' with M up to kAssocGridMaxDetections, a FINITE gate, and cell > 0 and finite.
inline void check_assoc_grid_args(double dt, bool have_det, long M, double gate, long rounds, double cell, bool have_out, long ld, long size) {
  const std::string pre = "target_estimation_amd: associate_grid: ";
  if (!(dt >= 0.0)) throw std::invalid_argument(pre + "dt must be >= 0, got " + std::to_string(dt));
  if (M < 0 || M > kAssocGridMaxDetections)
    throw std::invalid_argument(pre + "M must be 0.." + std::to_string(kAssocGridMaxDetections) + ", got " + std::to_string(M));
  if (M > 0 && !have_det) throw std::invalid_argument(pre + "the detections are required");
  if (!(gate > 0.0) || !(gate <= DBL_MAX)) throw std::invalid_argument(pre + "gate must be > 0 and finite, got " + std::to_string(gate));
  if (rounds < 1 || rounds > kAssocMaxRounds)
    throw std::invalid_argument(pre + "rounds must be 1.." + std::to_string(kAssocMaxRounds) + ", got " + std::to_string(rounds));
  if (!(cell > 0.0) || !(cell <= DBL_MAX)) throw std::invalid_argument(pre + "cell must be > 0 and finite, got " + std::to_string(cell));
  if (!have_out) throw std::invalid_argument(pre + "a required output is NULL");
  if (ld < size) throw std::invalid_argument(pre + "ld " + std::to_string(ld) + " < size " + std::to_string(size));
}
// one check for the host-side entry points that serve both forms: cell == 0 is the brute-force form
inline void check_assoc_args_for(double cell_or_0, double dt, bool have_det, long M, double gate, long rounds, bool have_out, long ld, long size) {
  if (cell_or_0 == 0.0) check_assoc_args(dt, have_det, M, gate, rounds, have_out, ld, size);
  else check_assoc_grid_args(dt, have_det, M, gate, rounds, cell_or_0, have_out, ld, size);
}

}  // namespace te
