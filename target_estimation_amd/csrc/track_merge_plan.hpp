// track_merge_plan.hpp -- no HIP: everything about "find and retire duplicate tracks" (target_batch_c.h,
// target_manager_find_duplicates_dev / target_manager_retire_duplicates) that is not a kernel -- the row, the
// eligibility classes, the pair cost and the pair box, the survivor rule, the argument checks.  track_merge.hip (the kernels),
// Shard / TargetManager (the host side) and tests/host/track_merge_plan_host_test.cpp (g++ alone) all build this header.  The
// inverse, d^2, the box, the cell map, the narrow limit, the hash and the keyed pick are associate[_grid]_plan.hpp's, unchanged.
#pragma once
#include <cfloat>
#include <cmath>

#include "associate_grid_plan.hpp"

namespace te {

constexpr int kMergeThreads = 256;   // threads of every track-merge workgroup: four wavefronts of 64

// THE ROW of a target: 80 bytes, the association's row with Sigma where that keeps W.  z is the association's zhat at the offset
// dt (NaN in z[0]: the association's row is invalid -- S = Sigma + R does not invert under assoc_invert_s); Sigma = (A(dt) P A(dt)^T
// + Q)[0:3, 0:3], upper triangle xx xy xz yy yz zz, the very doubles the table kernel forms BEFORE it adds R; tag as AssocRow's.
// One record, so that a visit of the self-scan reads one row and not two arrays.
struct MergeRow {
  double z[3];
  double Sigma[6];
  double tag;
};
static_assert(sizeof(MergeRow) == sizeof(AssocRow), "a merge row is a table row");

// row classes
constexpr int kMergeNone = 0;       // invalid, or fewer hits than min_hits: never a partner, never counted
constexpr int kMergeEligible = 1;   // valid, hits >= min_hits, narrow: binned, may be a partner
constexpr int kMergeWide = 2;       // valid, hits >= min_hits, not narrow: EXCLUDED (not brute-forced) and counted in info[3]

// A row is VALID iff the association's row is valid and Sigma's six words are finite: one validity rule for the project.
TE_ASSOC_HD inline bool merge_row_valid(const double* row) {
  bool ok = row[0] == row[0];
  for (int k = 0; k < 6; ++k) ok = ok && (row[3 + k] - row[3 + k] == 0.0);
  return ok;
}
// THE BOX OF A ROW: reach2_a = assoc_grid_reach2(gate, 2 Sigma_aa) -- the pair box of the row against a twin of itself (2 x is exact).
TE_ASSOC_HD inline void merge_row_reach2(const double* row, double gate, double* reach2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  reach2[0] = assoc_grid_reach2(gate, 2.0 * row[3]);
  reach2[1] = assoc_grid_reach2(gate, 2.0 * row[6]);
  reach2[2] = assoc_grid_reach2(gate, 2.0 * row[8]);
}
// THE CLASS.  A wide row is excluded, not brute-forced: a track whose box exceeds a cell is not known well enough to be merged
// with anything.  A large info[3] therefore says that `cell` is too small for the tracks' uncertainty.
TE_ASSOC_HD inline int merge_row_class(const double* row, int hits, int min_hits, double gate, double lim2) {
  if (!merge_row_valid(row)) return kMergeNone;
  if (hits < min_hits) return kMergeNone;
  double reach2[3];
  merge_row_reach2(row, gate, reach2);
  return (reach2[0] <= lim2 && reach2[1] <= lim2 && reach2[2] <= lim2) ? kMergeEligible : kMergeWide;
}

// THE PAIR of two eligible rows, ALWAYS ordered (lo, hi) by row index, so that both partners form the same bits:
//   C = Sigma_lo + Sigma_hi word by word in double; V = assoc_invert_s(C), an invalid C rejects; d2 = assoc_d2(z_lo, V, z_hi);
//   candidate iff d2 <= gate AND nu_a * nu_a <= assoc_grid_reach2(gate, C_aa) on every axis, nu_a = z_hi[a] - z_lo[a] the very
//   double assoc_d2 forms.  Plain multiplies, contraction off, no square root.
//
// WHY 27 CELLS SUFFICE.  fl(Sigma_lo + Sigma_hi) <= 2 max(Sigma_lo, Sigma_hi) exactly (the exact sum is at most that double, and
// rounding is monotone), and assoc_grid_reach2 is monotone in its second argument (two roundings of products by positive
// constants).  So the pair's reach2 never exceeds the larger of the two rows' reach2; both rows are narrow, so the pair's box
// satisfies reach2_a <= lim2, and associate_grid_plan.hpp's proved neighbour property holds for the pair with z_lo in the place
// of zhat and z_hi in the place of the detection (and, nu only changing sign, the other way round): the partner lies within +-1
// cell on every axis, and is found by walking 27 cells.  (tests/host/track_merge_plan_host_test.cpp checks the claim on random
// and adversarial Sigma: equal, one ulp apart, 2^60 apart, subnormal.)
TE_ASSOC_HD inline bool merge_pair_candidate(const double* row_lo, const double* row_hi, double gate, double* d2_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double C[6], V[6];
  for (int k = 0; k < 6; ++k) C[k] = row_lo[3 + k] + row_hi[3 + k];
  *d2_out = -1.0;
  if (!assoc_invert_s(C, V)) return false;
  const double nx = row_hi[0] - row_lo[0], ny = row_hi[1] - row_lo[1], nz = row_hi[2] - row_lo[2];
  const double d2 = assoc_d2(row_lo, V, row_hi[0], row_hi[1], row_hi[2]);
  *d2_out = d2;
  return d2 <= gate && nx * nx <= assoc_grid_reach2(gate, C[0]) && ny * ny <= assoc_grid_reach2(gate, C[3]) &&
         nz * nz <= assoc_grid_reach2(gate, C[5]);
}
// ... as row `self` meets row `other` on a walk
TE_ASSOC_HD inline bool merge_pair_candidate_of(const double* rows, int self, int other, double gate, double* d2_out) {
  const int lo = self < other ? self : other, hi = self < other ? other : self;
  return merge_pair_candidate(rows + (long)lo * kAssocRowWords, rows + (long)hi * kAssocRowWords, gate, d2_out);
}

// MATCHING: rounds of mutual best.  Every unmatched eligible row picks its best unmatched candidate partner by (d2, partner row)
// with assoc_take_keyed (repeats through hash collisions are harmless; a row never picks itself); two rows that picked each other
// are a pair.  A round is settled iff no row that had a candidate stayed unmatched in it.
// THE FIXED POINT is sorted greedy matching by (d2, lo, hi):
//   1. Let (lo, hi) be the smallest remaining pair under that key.  A candidate j of lo with d2(lo, j) < d2(lo, hi), or with
//      equal d2 and j < hi, would make {lo, j} the smaller pair (j < lo: its lower row is j < lo; lo < j < hi: same lower row, lower
//      upper row).  So lo picks hi; by the same argument with j < lo, hi picks lo.
//   2. So the smallest remaining pair is always mutual and is matched in the round it is seen in.
//   3. Matched rows leave, the rest is a smaller instance: the rounds take the pairs that sorted greedy takes, and no others.

// THE SURVIVOR: of a matched pair the WEAKER row is the duplicate: fewer hits; at equal hits more miss; at equal both the higher row.
TE_ASSOC_HD inline bool merge_is_weaker(int hits_self, int miss_self, int row_self, int hits_other, int miss_other, int row_other) {
  if (hits_self != hits_other) return hits_self < hits_other;
  if (miss_self != miss_other) return miss_self > miss_other;
  return row_self > row_other;
}

// THE REFUSALS that need no handle, in the order the header lists them (find: cap = 0, have_ids = true).
inline void check_merge_args(const char* what, bool have_info, double dt, double gate, long rounds, double cell, long min_hits, long n_batches,
                             bool have_per_batch, long cap, bool have_ids) {
  const std::string pre = std::string("target_estimation_amd: ") + what + ": ";
  if (!have_info) throw std::invalid_argument(pre + "info is required");
  if (!(dt >= 0.0)) throw std::invalid_argument(pre + "dt must be >= 0, got " + std::to_string(dt));
  if (!(gate > 0.0) || !(gate <= DBL_MAX)) throw std::invalid_argument(pre + "gate must be > 0 and finite, got " + std::to_string(gate));
  if (rounds < 1 || rounds > kAssocMaxRounds)
    throw std::invalid_argument(pre + "rounds must be 1.." + std::to_string(kAssocMaxRounds) + ", got " + std::to_string(rounds));
  if (!(cell > 0.0) || !(cell <= DBL_MAX)) throw std::invalid_argument(pre + "cell must be > 0 and finite, got " + std::to_string(cell));
  if (min_hits < 0 || min_hits > 255) throw std::invalid_argument(pre + "min_hits must be 0..255, got " + std::to_string(min_hits));
  if (n_batches < 0 || (n_batches > 0 && !have_per_batch)) throw std::invalid_argument(pre + "one output description per batch is needed");
  if (cap < 0 || (cap > 0 && !have_ids)) throw std::invalid_argument(pre + "retired_ids_out and kept_ids_out are required for cap > 0");
}
inline void check_merge_one_shard(const char* what, long shards) {
  if (shards > 1)
    throw std::runtime_error(std::string("target_estimation_amd: ") + what + ": the manager spans " + std::to_string(shards) +
                             " shards, so there is no single device that holds every target's row (not built: DESIGN 7)");
}

}  // namespace te
