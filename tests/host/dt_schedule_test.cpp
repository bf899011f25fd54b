// dt_schedule_test.cpp -- host checks of csrc/dt_schedule.hpp (no HIP): the clock accounting of a call with a time-step schedule,
// the key a recorded graph is filed under, and the view itself.  Built with g++ -fsanitize=address,undefined by
// tests/test_dt_schedule_host.py.  Prints "dt schedule tests ok" on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../target_estimation_amd/csrc/dt_schedule.hpp"

using te::DtSchedule;
using te::TClock;

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_clock(TClock a, TClock b) { return same_bits(a.hi, b.hi) && same_bits(a.lo, b.lo); }
static double ulp(double x) { return std::nextafter(std::fabs(x), INFINITY) - std::fabs(x); }

int main() {
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> f(0.25, 2.0);
  // ---- none: the default-constructed schedule, a null pointer whatever the length
  {
    DtSchedule none;
    CHECK(!none.on() && none.n == 0 && none.at(7, 0.004) == 0.004 && none.key().empty());
    DtSchedule null_with_length(nullptr, 20);
    CHECK(!null_with_length.on() && null_with_length.n == 0);
    CHECK(same_clock(none.advance(TClock{1.5, 1e-20}), TClock{1.5, 1e-20}));
    CHECK(!none.same_bits(std::vector<double>()));   // a scalar call's (empty) key never matches through same_bits
  }
  // ---- the clock over a schedule equals repeated te_clock_add, bit for bit, from clocks of every size (long uptimes included)
  for (double start : {0.0, 1.0, 86400.0, 3.0e7, -12.5}) {
    for (int n : {1, 2, 20, 600, 25000}) {
      std::vector<double> dt((size_t)n);
      for (double& d : dt) d = 0.004 * f(rng);
      dt[(size_t)n / 2] = 0.0;
      if (n > 3) dt[3] = 3 * 0.004;
      TClock want{start, 0.0};
      for (int s = 0; s < n; ++s) want = te::te_clock_add(want, dt[(size_t)s]);
      const DtSchedule sch(dt.data(), n);
      CHECK(sch.on() && sch.n == n && sch.at(n - 1, -1.0) == dt[(size_t)n - 1]);
      CHECK(same_clock(sch.advance(TClock{start, 0.0}), want));
      // served in parts (two calls): the same clock
      const long cut = n / 3;
      CHECK(same_clock(sch.part(cut, n - cut).advance(sch.part(0, cut).advance(TClock{start, 0.0})), want));
      CHECK(sch.part(cut, n - cut).n == n - cut && (n - cut == 0 || sch.part(cut, n - cut).at(0, -1.0) == dt[(size_t)cut]));
    }
  }
  // ---- an all-equal schedule lands within 1 ulp of te_clock_add_ticks (both are roundings of sums exact to about 2^-106)
  for (double start : {0.0, 0.123, 86400.0, 3.0e7}) {
    for (double d : {0.004, 1.0 / 250.0, 0.1, 1e-3 / 3.0, 0.0}) {
      for (int n : {1, 20, 600, 250 * 3600}) {
        const std::vector<double> dt((size_t)n, d);
        const TClock a = DtSchedule(dt.data(), n).advance(TClock{start, 0.0});
        const TClock b = te::te_clock_add_ticks(TClock{start, 0.0}, d, (double)n);
        const TClock zero{0.0, 0.0};
        const double ta = te::te_clock_time(zero, a), tb = te::te_clock_time(zero, b);
        CHECK(std::fabs(ta - tb) <= ulp(tb));
      }
    }
  }
  // ---- the key: values compared as bits
  {
    std::vector<double> dt(20);
    for (double& d : dt) d = 0.004 * f(rng);
    dt[5] = 0.0;
    const DtSchedule sch(dt.data(), 20);
    const std::vector<double> key = sch.key();
    CHECK(key.size() == 20 && sch.same_bits(key));
    std::vector<double> copy = dt;                      // another array, the same values: the same schedule
    CHECK(DtSchedule(copy.data(), 20).same_bits(key));
    copy[5] = -0.0;                                     // 0.0 == -0.0 as values, not as bits
    CHECK(copy[5] == dt[5] && !DtSchedule(copy.data(), 20).same_bits(key));
    copy = dt;
    copy[19] = std::nextafter(copy[19], 1.0);           // one changed entry, by one ulp
    CHECK(!DtSchedule(copy.data(), 20).same_bits(key));
    CHECK(!DtSchedule(dt.data(), 19).same_bits(key));   // a prefix
    copy = dt;
    copy[2] = std::nan("");                             // a NaN equals itself as bits: the recording is reused, not re-made every call
    const DtSchedule with_nan(copy.data(), 20);
    CHECK(with_nan.same_bits(with_nan.key()) && !with_nan.same_bits(key));
    // the cache's comparison: scalar recordings serve scalar calls, schedule recordings schedule calls
    const std::vector<double> eq(20, 0.004), empty;
    CHECK(te::dt_key_matches(empty, false, 0.004, DtSchedule(), 0.004));
    CHECK(!te::dt_key_matches(empty, false, 0.004, DtSchedule(), 0.005));
    CHECK(!te::dt_key_matches(empty, false, 0.004, DtSchedule(eq.data(), 20), 0.004));   // an all-equal schedule is not the scalar call
    CHECK(!te::dt_key_matches(eq, true, 0.0, DtSchedule(), 0.004));
    CHECK(te::dt_key_matches(eq, true, 0.0, DtSchedule(eq.data(), 20), 123.0));          // (the scalar is not read with a schedule)
    CHECK(te::dt_key_matches(key, true, 0.0, sch, 0.0) && !te::dt_key_matches(key, true, 0.0, DtSchedule(eq.data(), 20), 0.0));
  }
  static_assert((te::kDtTabMaxTicks - 1) * 8 < (1L << 32), "entry s of a table sits at a 32-bit byte offset");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("dt schedule tests ok\n");
  return 0;
}
