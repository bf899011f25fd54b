// Host checks of the shared-axes storage form (csrc/te_layout.hpp): the eligibility test on the shipped model files and on
// perturbed copies, and the record layout (one covariance block per kind of axis).  argv: the four model files.
#define __host__
#define __device__
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../target_estimation_amd/csrc/te_layout.hpp"
#include "../../target_estimation_amd/csrc/yaml_mini.hpp"

using namespace te;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class M>
static void check_layout(const char* name, int want_rw) {
  using S = Cfg<M, double, 1, LAYOUT_SEPARABLE_SHARED>;
  using P = Cfg<M, double, 1, LAYOUT_SEPARABLE_PACKED>;
  CHECK(S::SHARED && S::SEP && S::SEPPK && !P::SHARED);
  CHECK(S::RW == want_rw && S::RW < P::RW && S::X_OFF == S::PW && S::TPW == 64);
  CHECK(S::TILE_BYTES % 128 == 0 && S::TILE_BYTES >= 64L * S::RW * 8);
  CHECK(S::QR_WORDS == P::QR_WORDS);   // the (Q, R) row is the plain one
  std::set<int> words;
  for (int r = 0; r < M::N; ++r)
    for (int c = 0; c < M::N; ++c) {
      const int w = S::p_word(r, c);
      CHECK(w == S::PWORD.v[r][c]);
      if (group_of(M::TYPE, r) != group_of(M::TYPE, c)) { CHECK(w == -1 && P::p_word(r, c) == -1); continue; }
      CHECK(w >= 0 && w < S::PW);
      CHECK(w == S::p_word(c, r));                                                       // packed groups
      CHECK(w == S::p_word(share_rep(M::TYPE, r), share_rep(M::TYPE, c)));               // every axis of a kind -> the kind's block
      // two entries share a word only if they are the same entry of the blocks of two axes of one kind (or mirror images)
      for (int r2 = 0; r2 < M::N; ++r2)
        for (int c2 = 0; c2 < M::N; ++c2)
          if (S::p_word(r2, c2) == w) {
            const int a = share_rep(M::TYPE, r), b = share_rep(M::TYPE, c), a2 = share_rep(M::TYPE, r2), b2 = share_rep(M::TYPE, c2);
            CHECK((a == a2 && b == b2) || (a == b2 && b == a2));
          }
      words.insert(w);
    }
  CHECK((int)words.size() == S::PW);   // no unused word
  std::printf("layout %s: %d words (plain %d)\n", name, S::RW, P::RW);
}

int main(int argc, char** argv) {
  // share_rep: x, y, z of every model and roll, pitch, yaw of angular_rates fold onto the kind's first axis, state by state
  for (int r = 0; r < 6; ++r) CHECK(share_rep(UNIFORM_VELOCITY, r) == r - r % 3);
  for (int r = 0; r < 9; ++r) CHECK(share_rep(UNIFORM_ACCELERATION, r) == r - r % 3);
  for (int r = 0; r < 18; ++r) CHECK(share_rep(ANGULAR_RATES, r) == r - (r % 6) % 3);
  for (int r = 0; r < 12; ++r) CHECK(share_rep(ANGULAR_VELOCITIES, r) == ((r % 6) < 3 ? r - r % 3 : r));   // the attitude group is never shared
  check_layout<ModelAR>("angular_rates", 33);
  check_layout<ModelAV>("angular_velocities", 39);
  check_layout<ModelUA>("uniform_acceleration", 15);
  check_layout<ModelUV>("uniform_velocity", 9);

  CHECK(argc == 5);
  for (int i = 1; i < argc; ++i) {
    ModelFile mf;
    std::string err;
    CHECK(load_model_file(argv[i], mf, err));
    const int type = mf.type == "angular_rates" ? 0 : mf.type == "angular_velocities" ? 1 : mf.type == "uniform_acceleration" ? 2 : mf.type == "uniform_velocity" ? 3 : -1;
    CHECK(type >= 0);
    const int n = model_n(type), m = model_m(type);
    const std::vector<double> Q = mf.seqs["Q"], R = mf.seqs["R"], P = mf.seqs["P"];
    CHECK((int)Q.size() == n * n && (int)R.size() == m * m && (int)P.size() == n * n);
    // the shipped matrices are eligible
    CHECK(shared_axes_qr_ok(type, Q.data(), R.data()));
    CHECK(shared_axes_p0_ok(type, P.data(), 1));
    int refused = 0, kept = 0;
    const double up = 1.0 + 0x1p-52;   // one unit in the last place
    // every in-group entry of Q on a foldable axis: one ulp more on one axis alone ends it (exact comparison, no tolerance) ...
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        if (group_of(type, r) != group_of(type, c) || Q[r * n + c] == 0.0) continue;
        std::vector<double> Q2 = Q;
        Q2[r * n + c] *= up;
        const bool foldable = type != ANGULAR_VELOCITIES || (r % 6) < 3;
        CHECK(shared_axes_qr_ok(type, Q2.data(), R.data()) == !foldable);
        std::vector<double> P2 = P;
        if (P2[r * n + c] != 0.0) {
          P2[r * n + c] *= up;
          CHECK(shared_axes_p0_ok(type, P2.data(), 1) == !foldable);
          std::vector<double> three = P;   // ... also when it is the last of several initial covariances
          three.insert(three.end(), P.begin(), P.end());
          three.insert(three.end(), P2.begin(), P2.end());
          CHECK(shared_axes_p0_ok(type, three.data(), 2) && shared_axes_p0_ok(type, three.data(), 3) == !foldable);
        }
        foldable ? ++refused : ++kept;
      }
    for (int r = 0; r < m; ++r) {
      std::vector<double> R2 = R;
      R2[r * m + r] *= up;
      const bool foldable = type != ANGULAR_VELOCITIES || r < 3;
      CHECK(shared_axes_qr_ok(type, Q.data(), R2.data()) == !foldable);
    }
    // ... while the same factor on every axis of the kind keeps it
    std::vector<double> Q3 = Q;
    for (double& v : Q3) v *= 3.0;
    CHECK(shared_axes_qr_ok(type, Q3.data(), R.data()));
    CHECK(refused > 0 && (kept > 0) == (type == ANGULAR_VELOCITIES));
    std::printf("model %-22s perturbations refused %d, outside the shared kinds %d\n", mf.type.c_str(), refused, kept);
  }
  std::printf("%s\n", failures ? "SHARED AXES HOST TEST FAILED" : "shared axes host test ok");
  return failures ? 1 : 0;
}
