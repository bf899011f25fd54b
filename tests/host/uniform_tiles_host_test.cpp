// Host checks of the uniform-tile tables of the shared-axes storage form (csrc/te_layout.hpp Cfg::LIN): which record words are
// linear-chain covariance words (the words of a tile's block), and which 16-byte chunks hold nothing else (the chunks a uniform
// tile skips).  The tables are checked against the model structure itself, not against the code that builds them.
#define __host__
#define __device__
#include <cstdio>
#include <set>
#include <vector>

#include "../../target_estimation_amd/csrc/te_layout.hpp"

using namespace te;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class M>
static void check_tables(const char* name, int want_lw, const std::vector<int>& want_chunks, bool want_feature) {
  using S = Cfg<M, double, 1, LAYOUT_SEPARABLE_SHARED>;
  using P = Cfg<M, double, 1, LAYOUT_SEPARABLE_PACKED>;
  using F = Cfg<M, float, 1, LAYOUT_SEPARABLE_PACKED>;
  CHECK(S::UT == want_feature && !P::UT && !F::UT);        // fp32 and plain batches: compiled out
  CHECK(P::LW == 0 && P::LIN_CHUNKS == 0 && F::LW == 0);
  // the linear P words, from the model: P(r, c) with r and c states of one [p v (a)] chain -- any row of a linear model, the
  // x, y, z rows (r % 6 < 3) of the EKF
  std::set<int> lin, other;
  for (int r = 0; r < M::N; ++r)
    for (int c = 0; c < M::N; ++c) {
      const int w = S::p_word(r, c);
      if (w < 0) continue;
      const bool chain = !M::EKF || ((r % 6) < 3 && (c % 6) < 3);
      (chain ? lin : other).insert(w);
    }
  for (int w : lin) CHECK(other.count(w) == 0);
  CHECK((int)lin.size() == want_lw && S::LW == want_lw);
  int k = 0;
  for (int w = 0; w < S::RW; ++w) {
    if (lin.count(w)) { CHECK(S::LIN.idx[w] == k && S::LIN.w[k] == w); ++k; }   // block order = record order
    else CHECK(S::LIN.idx[w] == -1);
  }
  // x and the unwrap memory are never block words
  for (int w = S::X_OFF; w < S::RW; ++w) CHECK(S::LIN.idx[w] == -1);
  // a chunk is skipped iff both of its words are linear P words; the tail word belongs to no chunk
  std::vector<int> chunks;
  for (int c = 0; c < S::NC; ++c) {
    const bool all = lin.count(2 * c) && lin.count(2 * c + 1);
    CHECK(S::lin_chunk(c) == all);
    if (all) chunks.push_back(c);
  }
  CHECK(chunks == want_chunks && S::LIN_CHUNKS == (int)want_chunks.size());
  CHECK(S::VW == 2 && 2 * S::NC + S::REM1 == S::RW);
  std::printf("uniform tiles %s: %d block words, %d skipped chunks of %d, feature %s\n", name, S::LW, S::LIN_CHUNKS, S::NC, S::UT ? "on" : "off");
}

int main() {
  check_tables<ModelAR>("angular_rates", 12, {0, 1, 2, 3, 4, 5}, true);
  check_tables<ModelUA>("uniform_acceleration", 6, {0, 1, 2}, true);
  check_tables<ModelUV>("uniform_velocity", 3, {0}, true);             // P(0,0), P(0,3); P(3,3) shares its chunk with x
  check_tables<ModelAV>("angular_velocities", 3, {0}, false);          // P(0,0), P(0,6); the kernels are built without the feature
  {
    using S = Cfg<ModelAV, double, 1, LAYOUT_SEPARABLE_SHARED>;
    CHECK(S::LIN.w[0] == S::p_word(0, 0) && S::LIN.w[1] == S::p_word(0, 6) && S::LIN.w[2] == S::p_word(6, 6));
    using U = Cfg<ModelUV, double, 1, LAYOUT_SEPARABLE_SHARED>;
    CHECK(U::LIN.w[0] == U::p_word(0, 0) && U::LIN.w[1] == U::p_word(0, 3) && U::LIN.w[2] == U::p_word(3, 3) && U::X_OFF == 3);
  }
  CHECK(uniform_tiles_model(ANGULAR_RATES) && uniform_tiles_model(UNIFORM_ACCELERATION) && uniform_tiles_model(UNIFORM_VELOCITY));
  std::printf("%s\n", failures ? "UNIFORM TILES HOST TEST FAILED" : "uniform tiles host test ok");
  return failures ? 1 : 0;
}
