// CPU-only test of csrc/associate_plan.hpp, the HIP-free half of the association of unlabelled detections: the refusal table, the
// grid plan (every (row, column) pair belongs to exactly one workgroup, for awkward sizes and forced chunk counts), the tie rule of
// a partial minimum and of the merge, the inverse of S and its validity rule, d^2.  g++ alone, sanitised, contraction off.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../target_estimation_amd/csrc/associate_plan.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

template <class F>
static bool refused(F&& f) {
  try { f(); } catch (const std::invalid_argument&) { return true; } catch (const std::runtime_error&) { return true; }
  return false;
}

static void test_refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(!refused([&] { te::check_assoc_args(0.01, true, 10, 9.0, 4, true, 16, 16); }));
  CHECK(!refused([&] { te::check_assoc_args(0.0, true, 10, inf, 1, true, 16, 10); }));                  // dt 0, gate +inf, ld > size
  CHECK(!refused([&] { te::check_assoc_args(0.01, false, 0, 9.0, te::kAssocMaxRounds, true, 0, 0); })); // M == 0 needs no detections
  CHECK(!refused([&] { te::check_assoc_args(0.01, true, te::kAssocMaxDetections, 9.0, 4, true, 1, 1); }));
  CHECK(refused([&] { te::check_assoc_args(-0.01, true, 10, 9.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(nan, true, 10, 9.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, -1, 9.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, te::kAssocMaxDetections + 1, 9.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, false, 3, 9.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, 0.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, -1.0, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, nan, 4, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, 9.0, 0, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, 9.0, te::kAssocMaxRounds + 1, true, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, 9.0, 4, false, 16, 16); }));
  CHECK(refused([&] { te::check_assoc_args(0.01, true, 10, 9.0, 4, true, 15, 16); }));
  CHECK(!refused([&] { te::check_assoc_one_shard(1); }));
  CHECK(refused([&] { te::check_assoc_one_shard(2); }));
  CHECK(te::assoc_forced_chunks_from(nullptr) == 0 && te::assoc_forced_chunks_from("") == 0 && te::assoc_forced_chunks_from("x") == 0);
  CHECK(te::assoc_forced_chunks_from("0") == 0 && te::assoc_forced_chunks_from("-3") == 0 && te::assoc_forced_chunks_from("3") == 3);
  CHECK(te::assoc_forced_chunks_from("100000") == te::kAssocMaxChunks);
}

// every (row, column) pair is covered exactly once: walk the grid as the scan kernels do
static void cover(long rows, long cols, int forced) {
  const te::AssocGrid g = te::plan_assoc_grid(rows, cols, forced);
  CHECK(g.chunks >= 1 && g.chunks <= te::kAssocMaxChunks);
  CHECK((long)g.row_tiles * te::kAssocTile >= rows && ((long)g.row_tiles - 1) * te::kAssocTile < (rows > 0 ? rows : 1));
  if (forced > 0) CHECK(g.chunks == (forced > te::kAssocMaxChunks ? te::kAssocMaxChunks : forced));
  std::vector<int> col_seen((size_t)cols, 0);
  long last_end = 0;
  for (int c = 0; c < g.chunks; ++c) {
    const long b = g.col_begin(c), e = g.col_end(c);
    CHECK(b <= e && e <= cols && b == last_end);   // ascending, contiguous: the merge order is the index order
    last_end = e;
    for (long j = b; j < e; j += te::kAssocTile)
      for (long t = j; t < e && t < j + te::kAssocTile; ++t) ++col_seen[(size_t)t];
  }
  CHECK(last_end == cols);
  for (long j = 0; j < cols; ++j) CHECK(col_seen[(size_t)j] == 1);
  std::vector<int> row_seen((size_t)rows, 0);
  for (int t = 0; t < g.row_tiles; ++t)
    for (int k = 0; k < te::kAssocTile; ++k) {
      const long r = (long)t * te::kAssocTile + k;
      if (r < rows) ++row_seen[(size_t)r];
    }
  for (long r = 0; r < rows; ++r) CHECK(row_seen[(size_t)r] == 1);
}

static void test_grid() {
  const long sizes[] = {0, 1, 63, 64, 65, 130, 255, 256, 257, 300, 1000, 4096, 10000, 65536};
  for (long rows : sizes)
    for (long cols : sizes)
      for (int forced : {0, 1, 2, 3, 7, 64, 1000}) cover(rows, cols, forced);
  cover(1000000, 4096, 0);
  // the planned grid reaches the device: 10^4 x 10^4 is 40 row tiles, so the columns are cut
  const te::AssocGrid g = te::plan_assoc_grid(10000, 10000, 0);
  CHECK(g.row_tiles == 40 && g.chunks > 1 && (long)g.row_tiles * g.chunks >= 256 && g.chunk_len % te::kAssocTile == 0);
  const te::AssocGrid big = te::plan_assoc_grid(1000000, 4096, 0);
  CHECK(big.chunks == 1);                          // the rows alone fill it
  const te::AssocGrid mirror = te::plan_assoc_grid(4096, 1000000, 0);
  CHECK(mirror.row_tiles == 16 && mirror.chunks == te::kAssocMaxChunks);
  const te::AssocGrid tiny = te::plan_assoc_grid(5, 3, 0);
  CHECK(tiny.chunks == 1 && tiny.row_tiles == 1);
}

static void test_tie_rule() {
  te::AssocBest b = te::assoc_best_none();
  CHECK(b.idx == -1);
  te::assoc_take(b, 5.0, 7);
  CHECK(b.idx == 7 && b.d2 == 5.0);
  te::assoc_take(b, 5.0, 9);          // equal: the earlier (lower) index stays
  CHECK(b.idx == 7);
  te::assoc_take(b, 4.0, 11);
  CHECK(b.idx == 11 && b.d2 == 4.0);
  const double inf = std::numeric_limits<double>::infinity();
  te::AssocBest c = te::assoc_best_none();
  te::assoc_take(c, inf, 3);          // +inf is a cost like any other under gate = +inf
  CHECK(c.idx == 3 && c.d2 == inf);
  CHECK(te::assoc_candidate(inf, inf) && te::assoc_candidate(2.0, 2.0) && !te::assoc_candidate(std::nextafter(2.0, 3.0), 2.0));
  CHECK(!te::assoc_candidate(std::numeric_limits<double>::quiet_NaN(), inf));
  // the merge: 3 chunks x 4 entries, chunk-major; equal costs across chunks -> the lower chunk (lower indices) wins
  const long ld = 4;
  const double d2[12] = {3.0, -1.0, 2.0, -1.0,   3.0, 1.0, 2.5, -1.0,   2.0, 1.0, 2.0, -1.0};
  const int idx[12] = {0, -1, 1, -1,   5, 6, 4, -1,   9, 8, 10, -1};
  CHECK(te::assoc_merge(d2, idx, ld, 3, 0).idx == 9);    // strictly smaller in the last chunk
  CHECK(te::assoc_merge(d2, idx, ld, 3, 1).idx == 6);    // none in chunk 0; 1.0 == 1.0: chunk 1 stays
  CHECK(te::assoc_merge(d2, idx, ld, 3, 2).idx == 1);    // 2.0 in chunk 0 and chunk 2: chunk 0 stays
  CHECK(te::assoc_merge(d2, idx, ld, 3, 3).idx == -1);
  CHECK(te::assoc_merge(d2, idx, ld, 1, 1).idx == -1);
}

static void test_inverse() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double W[6];
  const double I[6] = {1, 0, 0, 1, 0, 1};
  CHECK(te::assoc_invert_s(I, W));
  for (int k = 0; k < 6; ++k) CHECK(W[k] == I[k]);
  const double S[6] = {4.0, 1.0, 0.5, 3.0, 0.25, 2.0};
  CHECK(te::assoc_invert_s(S, W));
  const double Sf[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
  const double Wf[3][3] = {{W[0], W[1], W[2]}, {W[1], W[3], W[4]}, {W[2], W[4], W[5]}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double v = 0;
      for (int k = 0; k < 3; ++k) v += Sf[r][k] * Wf[k][c];
      CHECK(std::fabs(v - (r == c ? 1.0 : 0.0)) < 1e-15);
    }
  const double bad[][6] = {{1, 0, 0, -1, 0, 1}, {1, 0, 0, 0, 0, 1}, {0, 0, 0, 1, 0, 1}, {1, 2, 0, 1, 0, 1} /* det -3 */,
                           {1, 1, 0, 1, 0, 1} /* det 0 */, {inf, 0, 0, 1, 0, 1}, {1, nan, 0, 1, 0, 1}, {1, 0, 0, 1, 0, nan},
                           {1e200, 0, 0, 1e200, 0, 1e200} /* det overflows */};
  for (const auto& b : bad) {
    CHECK(!te::assoc_invert_s(b, W));
    for (int k = 0; k < 6; ++k) CHECK(W[k] != W[k]);
  }
  // d^2: the unit form is the squared distance exactly on integers; a NaN anywhere gives NaN
  const double z[3] = {1.0, 2.0, 3.0};
  CHECK(te::assoc_d2(z, I, 4.0, 6.0, 3.0) == 25.0);
  CHECK(te::assoc_d2(z, I, 1.0, 2.0, 3.0) == 0.0);
  const double d = te::assoc_d2(z, I, nan, 6.0, 3.0);
  CHECK(d != d);
  te::AssocRow row{};
  CHECK(sizeof(row) == 80);
}

int main() {
  test_refusals();
  test_grid();
  test_tie_rule();
  test_inverse();
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("associate plan host test ok\n");
  return 0;
}
