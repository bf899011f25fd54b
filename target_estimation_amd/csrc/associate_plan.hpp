// associate_plan.hpp -- no HIP: everything about "associate unlabelled detections with targets" (target_batch_c.h,
// target_batch_associate*) that is not a kernel -- the table row, the inverse of S and its validity rule, the pair cost d^2, the
// candidate rule, the partial minimum and its merge, the grid plan of the two scans, the argument checks.  associate.hip (the
// kernels), Batch / Shard / TargetManager (the host side) and tests/host/associate_plan_host_test.cpp (g++ alone) all build this header.
#pragma once
#include <cmath>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <string>

#if defined(__HIPCC__)
#define TE_ASSOC_HD __host__ __device__
#else
#define TE_ASSOC_HD
#endif

namespace te {

constexpr long kAssocMaxDetections = 65536;   // TARGET_ASSOC_MAX_DETECTIONS
constexpr int kAssocMaxRounds = 16;           // TARGET_ASSOC_MAX_ROUNDS
constexpr int kAssocTile = 256;               // threads of a scan workgroup = the rows (columns) it owns = the entries staged per LDS tile
constexpr int kAssocMaxChunks = 64;           // the most column chunks a scan is cut into (and the most TE_ASSOC_COL_CHUNKS may force)
constexpr int kAssocTargetWgs = 1024;         // workgroups a scan aims for: four per CU of a 256-CU device
constexpr int kAssocRowWords = 10;            // doubles of a table row: zhat (3) | W = S^-1 upper triangle xx xy xz yy yz zz (6) | tag (1)

// THE TABLE ROW of a target: 80 bytes.  tag carries (batch << 32 | slot) as the bits of the tenth double, so that a detection's
// match (a row of the call's concatenated table) translates back to (batch, slot) without a table of batch offsets.
struct AssocRow {
  double z[3];
  double W[6];
  double tag;
};
static_assert(sizeof(AssocRow) == kAssocRowWords * sizeof(double), "a table row is 80 bytes");

// THE INVERSE W = S^-1 of the symmetric 3 x 3 innovation covariance S (upper triangle xx xy xz yy yz zz), in double, by
// cofactors: symmetric by construction, 6 words.  Returns false -- the slot is never a candidate and its row is NaN -- when S is not
// finite, has a non-positive diagonal entry or a non-positive determinant (a NaN determinant fails the comparison).
TE_ASSOC_HD inline bool assoc_invert_s(const double* S, double* W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && (S[k] - S[k] == 0.0);   // finite: inf - inf and NaN - NaN are NaN
  ok = ok && S[0] > 0.0 && S[3] > 0.0 && S[5] > 0.0;
  const double c00 = S[3] * S[5] - S[4] * S[4];
  const double c01 = S[2] * S[4] - S[1] * S[5];
  const double c02 = S[1] * S[4] - S[2] * S[3];
  const double c11 = S[0] * S[5] - S[2] * S[2];
  const double c12 = S[1] * S[2] - S[0] * S[4];
  const double c22 = S[0] * S[3] - S[1] * S[1];
  const double det = (S[0] * c00 + S[1] * c01) + S[2] * c02;
  ok = ok && det > 0.0 && (det - det == 0.0);
  if (!ok) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 6; ++k) W[k] = nan;
    return false;
  }
  W[0] = c00 / det; W[1] = c01 / det; W[2] = c02 / det;
  W[3] = c11 / det; W[4] = c12 / det; W[5] = c22 / det;
  return true;
}

// THE PAIR COST d^2 = nu^T W nu, nu = z - zhat, in double: ONE function for both scan orientations, plain multiplies and adds in
// this order with contraction off, so that the two scans give the same bits for the same pair.
TE_ASSOC_HD inline double assoc_d2(const double* zhat, const double* W, double x, double y, double z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nx = x - zhat[0], ny = y - zhat[1], nz = z - zhat[2];
  const double t0 = (W[0] * nx + W[1] * ny) + W[2] * nz;
  const double t1 = (W[1] * nx + W[3] * ny) + W[4] * nz;
  const double t2 = (W[2] * nx + W[4] * ny) + W[5] * nz;
  return (nx * t0 + ny * t1) + nz * t2;
}
// THE CANDIDATE RULE: <=, so a NaN cost (a NaN in either operand) rejects; gate may be +inf
TE_ASSOC_HD inline bool assoc_candidate(double d2, double gate) { return d2 <= gate; }

// A PARTIAL MINIMUM: the best candidate a scan has seen for its row (column) over some ascending range of the other index.
// idx == -1: none.  A scan walks its range in ascending order and takes a candidate only when it is STRICTLY smaller; the
// resolve step merges the chunks' partials in ascending chunk order by the same rule -- so among equal costs the lowest index wins:
// the tie rule (d^2, detection) of a target's pick and (d^2, batch, slot) of a detection's (rows are concatenated in batch order).
struct AssocBest {
  double d2;
  int idx;
};
TE_ASSOC_HD inline AssocBest assoc_best_none() { return AssocBest{-1.0, -1}; }
TE_ASSOC_HD inline void assoc_take(AssocBest& best, double d2, int idx) {
  if (best.idx < 0 || d2 < best.d2) { best.d2 = d2; best.idx = idx; }
}
// the merge of n_chunks partials of entry e, stored chunk-major with leading dimension ld
TE_ASSOC_HD inline AssocBest assoc_merge(const double* part_d2, const int* part_idx, long ld, int n_chunks, long e) {
  AssocBest best = assoc_best_none();
  for (int c = 0; c < n_chunks; ++c) {
    const int idx = part_idx[(long)c * ld + e];
    if (idx >= 0) assoc_take(best, part_d2[(long)c * ld + e], idx);
  }
  return best;
}

// THE GRID of a scan: row tiles x column chunks.  A workgroup owns kAssocTile consecutive rows and walks the columns
// [col_begin(c), col_end(c)) of its chunk c; every (row, column) pair belongs to exactly one workgroup.  The chunk count makes the
// grid reach kAssocTargetWgs workgroups where the rows alone do not (10^4 rows are 40 tiles), without cutting a chunk below one LDS
// tile of columns; forced > 0 (TE_ASSOC_COL_CHUNKS) sets it regardless, so that small calls exercise the merge -- chunks beyond the
// columns are then empty.
struct AssocGrid {
  long rows = 0, cols = 0;
  int row_tiles = 0;
  int chunks = 1;
  long chunk_len = 0;
  TE_ASSOC_HD long col_begin(int c) const { const long b = (long)c * chunk_len; return b < cols ? b : cols; }
  TE_ASSOC_HD long col_end(int c) const { const long e = (long)(c + 1) * chunk_len; return e < cols ? e : cols; }
};
inline AssocGrid plan_assoc_grid(long rows, long cols, int forced) {
  AssocGrid g;
  g.rows = rows < 0 ? 0 : rows;
  g.cols = cols < 0 ? 0 : cols;
  g.row_tiles = (int)((g.rows + kAssocTile - 1) / kAssocTile);
  int chunks;
  if (forced > 0) {
    chunks = forced > kAssocMaxChunks ? kAssocMaxChunks : forced;
  } else {
    const long col_tiles = (g.cols + kAssocTile - 1) / kAssocTile;
    long want = g.row_tiles > 0 ? (kAssocTargetWgs + g.row_tiles - 1) / g.row_tiles : 1;
    if (want > col_tiles) want = col_tiles;
    if (want > kAssocMaxChunks) want = kAssocMaxChunks;
    chunks = want < 1 ? 1 : (int)want;
  }
  g.chunks = chunks;
  g.chunk_len = (g.cols + chunks - 1) / chunks;
  if (forced <= 0 && g.chunk_len > 0) {   // whole LDS tiles per chunk, then no more chunks than still have columns
    g.chunk_len = (g.chunk_len + kAssocTile - 1) / kAssocTile * kAssocTile;
    g.chunks = (int)((g.cols + g.chunk_len - 1) / g.chunk_len);
  }
  if (g.chunks < 1) g.chunks = 1;
  return g;
}
// TE_ASSOC_COL_CHUNKS as read from the environment: 0 (null or junk) = planned, else 1 .. kAssocMaxChunks
inline int assoc_forced_chunks_from(const char* env) {
  if (!env || !env[0]) return 0;
  char* end = nullptr;
  const long v = std::strtol(env, &end, 10);
  if (end == env || v < 1) return 0;
  return v > kAssocMaxChunks ? kAssocMaxChunks : (int)v;
}

// THE REFUSALS.  have_det: the detections were given (required when M > 0); have_out: every required output was given; ld, size:
// the leading dimension of meas_out against the batch's size (pass ld = size where no batch is at hand yet).  Throws
// std::invalid_argument; the caller has enqueued nothing yet.
inline void check_assoc_args(double dt, bool have_det, long M, double gate, long rounds, bool have_out, long ld, long size) {
  const std::string pre = "target_estimation_amd: associate: ";
  if (!(dt >= 0.0)) throw std::invalid_argument(pre + "dt must be >= 0, got " + std::to_string(dt));
  if (M < 0 || M > kAssocMaxDetections)
    throw std::invalid_argument(pre + "M must be 0.." + std::to_string(kAssocMaxDetections) + ", got " + std::to_string(M));
  if (M > 0 && !have_det) throw std::invalid_argument(pre + "the detections are required");
  if (!(gate > 0.0)) throw std::invalid_argument(pre + "gate must be > 0 (+inf switches it off), got " + std::to_string(gate));
  if (rounds < 1 || rounds > kAssocMaxRounds)
    throw std::invalid_argument(pre + "rounds must be 1.." + std::to_string(kAssocMaxRounds) + ", got " + std::to_string(rounds));
  if (!have_out) throw std::invalid_argument(pre + "a required output is NULL");
  if (ld < size) throw std::invalid_argument(pre + "ld " + std::to_string(ld) + " < size " + std::to_string(size));
}
// ... and of the manager forms, which leave their result on ONE device
inline void check_assoc_one_shard(long shards) {
  if (shards > 1)
    throw std::runtime_error("target_estimation_amd: associate: the manager spans " + std::to_string(shards) +
                             " shards, so there is no single device that holds every target's row (not built: DESIGN 7)");
}

}  // namespace te
