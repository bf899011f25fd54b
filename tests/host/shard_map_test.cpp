// shard_map_test.cpp -- host checks of csrc/shard_map.hpp (placement rule, merged enumeration, rank_of_slot) and of
// csrc/row_split.hpp (the gather / scatter of a host-array call split by shard or by batch), built with
// g++ -fsanitize=address,undefined by tests/test_shard_map_host.py.  Prints "shard map tests ok" on success.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../target_estimation_amd/csrc/row_split.hpp"
#include "../../target_estimation_amd/csrc/shard_map.hpp"

using te::ShardMap;

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
  } while (0)

// the rule for one creation, restated: fewest of the model, ties to the lowest index
static int brute_one(const ShardMap& m, int model) {
  int best = 0;
  for (int s = 0; s < m.shards(); ++s)
    if (m.count(s, model) < m.count(best, model)) best = s;
  return best;
}

static void create_batch(ShardMap& m, int model, const std::vector<unsigned>& ids) {
  const std::vector<int> where = m.place_batch(model, (long)ids.size());
  for (size_t i = 0; i < ids.size(); ++i) m.insert(ids[i], where[i], model);
}

static void test_single_creations() {
  ShardMap m;
  m.reset(3);
  // models interleave: each model balances on its own
  for (unsigned id = 0; id < 30; ++id) {
    const int model = (int)(id % 2 == 0 ? 3 : 0);
    const int k = m.place_one(model);
    CHECK(k == brute_one(m, model));
    m.insert(id, k, model);
  }
  for (int s = 0; s < 3; ++s) CHECK(m.count(s, 3) == 5 && m.count(s, 0) == 5);
  CHECK(m.shard_of(0) == 0 && m.shard_of(2) == 1 && m.shard_of(4) == 2 && m.shard_of(1) == 0 && m.shard_of(3) == 1);
  CHECK(m.shard_of(999) == -1);
}

static void test_batched_runs() {
  ShardMap m;
  m.reset(3);
  // 10 ids into empty shards: 4, 3, 3 in contiguous runs, in the caller's order
  std::vector<unsigned> ids;
  for (unsigned i = 0; i < 10; ++i) ids.push_back(100 + i * 7);
  const std::vector<int> w = m.place_batch(2, 10);
  const int want[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 2};
  for (int i = 0; i < 10; ++i) CHECK(w[(size_t)i] == want[i]);
  create_batch(m, 2, ids);
  // a second batch of the same model fills the lowest shards first: counts 4,3,3 + 5 -> 5,5,5
  std::vector<unsigned> ids2 = {1, 2, 3, 4, 5};
  const std::vector<int> w2 = m.place_batch(2, 5);
  CHECK(w2 == std::vector<int>({0, 1, 1, 2, 2}));
  create_batch(m, 2, ids2);
  for (int s = 0; s < 3; ++s) CHECK(m.count(s, 2) == 5);
  // a batch of another model starts from its own (empty) counts
  CHECK(m.place_batch(1, 2) == std::vector<int>({0, 1}));
  // the counts a batch reaches are those of single creations in a row, for random starting points
  std::mt19937 rng(7);
  for (int trial = 0; trial < 200; ++trial) {
    ShardMap a, b;
    const int n = 1 + (int)(rng() % 8);
    a.reset(n); b.reset(n);
    unsigned next = 0;
    for (int s = 0; s < n; ++s) {
      const int pre = (int)(rng() % 6);
      for (int j = 0; j < pre; ++j) { a.insert(next, s, 0); b.insert(next, s, 0); ++next; }
    }
    const long k = (long)(rng() % 40);
    const std::vector<int> w3 = a.place_batch(0, k);
    for (long j = 0; j + 1 < k; ++j) CHECK(w3[(size_t)j] <= w3[(size_t)j + 1]);   // contiguous runs in shard order
    for (long j = 0; j < k; ++j) a.insert(next + (unsigned)j, w3[(size_t)j], 0);
    for (long j = 0; j < k; ++j) b.insert(next + (unsigned)j, b.place_one(0), 0);
    for (int s = 0; s < n; ++s) CHECK(a.count(s, 0) == b.count(s, 0));
  }
}

static void test_erase_and_recreate() {
  ShardMap m;
  m.reset(2);
  create_batch(m, 3, {10, 11, 12, 13});   // 10, 11 -> 0; 12, 13 -> 1
  CHECK(m.shard_of(10) == 0 && m.shard_of(13) == 1);
  CHECK(m.erase(10) && m.erase(11));
  CHECK(!m.erase(11));
  CHECK(m.size() == 2 && m.count(0, 3) == 0 && m.count(1, 3) == 2);
  // re-created ids go where the rule says now: shard 0 is empty
  CHECK(m.place_one(3) == 0);
  m.insert(12 + 100, m.place_one(3), 3);
  create_batch(m, 3, {10, 11, 20});        // counts 1, 2 -> 3 new: shard 0 takes 2, shard 1 takes 1
  CHECK(m.shard_of(10) == 0 && m.shard_of(11) == 0 && m.shard_of(20) == 1);
  CHECK(m.count(0, 3) == 3 && m.count(1, 3) == 3);
}

// a toy manager: shards of batches of slot ids, erase by swap with the last slot, batched compaction
struct ToyBatch { std::vector<unsigned> slots; };
static void erase_swap(ToyBatch& b, unsigned id) {
  auto it = std::find(b.slots.begin(), b.slots.end(), id);
  if (it == b.slots.end()) return;
  *it = b.slots.back();
  b.slots.pop_back();
}
static void erase_compact(ToyBatch& b, const std::vector<unsigned>& ids) {   // the survivors keep their order
  std::vector<unsigned> keep;
  for (unsigned id : b.slots)
    if (std::find(ids.begin(), ids.end(), id) == ids.end()) keep.push_back(id);
  b.slots = keep;
}

static void check_ranks(const std::vector<std::vector<ToyBatch>>& shards) {
  std::vector<std::vector<unsigned>> lists;
  std::vector<unsigned> brute;
  for (const auto& sh : shards) {
    std::vector<unsigned> l;
    for (const auto& b : sh) l.insert(l.end(), b.slots.begin(), b.slots.end());
    brute.insert(brute.end(), l.begin(), l.end());
    std::sort(l.begin(), l.end());
    lists.push_back(l);
  }
  std::sort(brute.begin(), brute.end());
  const std::vector<unsigned> merged = te::merge_sorted_ids(lists);
  CHECK(merged == brute);
  CHECK(std::is_sorted(merged.begin(), merged.end()));
  // every slot's rank = its id's position in the brute-force sort; the ranks are a permutation of 0..N-1
  std::vector<int> seen(brute.size(), 0);
  for (const auto& sh : shards)
    for (const auto& b : sh) {
      std::vector<int> r(b.slots.size());
      te::ranks_of_slots(merged, b.slots.data(), (long)b.slots.size(), r.data());
      for (size_t s = 0; s < b.slots.size(); ++s) {
        long pos = -1;
        for (size_t q = 0; q < brute.size(); ++q) if (brute[q] == b.slots[s]) pos = (long)q;
        CHECK(r[s] == pos);
        if (r[s] >= 0) ++seen[(size_t)r[s]];
      }
    }
  for (int c : seen) CHECK(c == 1);
}

static void test_ranks() {
  std::mt19937 rng(11);
  std::vector<std::vector<ToyBatch>> shards(3, std::vector<ToyBatch>(2));
  std::vector<unsigned> ids(600);
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = (unsigned)(i * 37 % 1009) + 5;
  std::shuffle(ids.begin(), ids.end(), rng);
  for (size_t i = 0; i < ids.size(); ++i) shards[i % 3][(i / 3) % 2].slots.push_back(ids[i]);
  check_ranks(shards);
  for (int k = 0; k < 40; ++k) erase_swap(shards[(size_t)k % 3][(size_t)k % 2], ids[(size_t)(k * 7)]);   // erase by swap
  check_ranks(shards);
  std::vector<unsigned> gone(ids.begin() + 300, ids.begin() + 420);
  for (auto& sh : shards) for (auto& b : sh) erase_compact(b, gone);             // batched compaction
  check_ranks(shards);
  // an id that is not in the list has rank -1
  std::vector<unsigned> all = {1, 4, 9};
  unsigned q[3] = {4, 5, 9};
  int r[3];
  te::ranks_of_slots(all, q, 3, r);
  CHECK(r[0] == 1 && r[1] == -1 && r[2] == 2);
}

// gather -> scatter over a split of n rows into parts: every width from 1 to n * n, null arrays, empty position lists
static void test_row_split() {
  std::mt19937 rng(23);
  const long n = 7;
  for (long w : {1L, 2L, 6L, 7L, n * n}) {
    std::vector<double> a((size_t)(n * w));
    for (size_t i = 0; i < a.size(); ++i) a[i] = (double)i + 0.5;
    // a split as splitIds makes it: every position in exactly one part or in `unknown`, the caller's order kept inside a part
    te::Split sp;
    sp.src.resize(3);
    for (long i = 0; i < n; ++i) {
      const unsigned k = rng() % 4;
      if (k == 3) sp.unknown.push_back(i); else sp.src[k].push_back(i);
    }
    std::vector<double> back((size_t)(n * w), -1.0);
    for (const auto& pos : sp.src) {
      const std::vector<double> rows = te::gatherRows(a.data(), pos, w);
      CHECK(rows.size() == pos.size() * (size_t)w);
      for (size_t j = 0; j < pos.size(); ++j)
        for (long c = 0; c < w; ++c) CHECK(rows[j * (size_t)w + (size_t)c] == a[(size_t)(pos[j] * w + c)]);
      te::scatterRows(back.data(), rows, pos, w);
    }
    for (long i = 0; i < n; ++i) {   // the round trip restores every row that belongs to a part and touches no other
      const bool unknown = std::find(sp.unknown.begin(), sp.unknown.end(), i) != sp.unknown.end();
      for (long c = 0; c < w; ++c) CHECK(back[(size_t)(i * w + c)] == (unknown ? -1.0 : a[(size_t)(i * w + c)]));
    }
    // null arrays: nothing gathered, nothing written
    CHECK(te::gatherRows((const double*)nullptr, sp.src[0], w).empty());
    te::scatterRows((double*)nullptr, std::vector<double>(), sp.src[0], w);
    // empty position lists
    const std::vector<long> none;
    CHECK(te::gatherRows(a.data(), none, w).empty());
    std::vector<double> untouched = back;
    te::scatterRows(back.data(), std::vector<double>(), none, w);
    CHECK(back == untouched);

    // RowsIn / RowsOut: pos == null is the caller's array itself, a null array stays null, a packed output comes back at pos
    const std::vector<long> pos = {5, 0, 3};
    te::RowsIn<double> whole(a.data(), nullptr, w), packed(a.data(), &pos, w), absent((const double*)nullptr, &pos, w);
    CHECK(whole.get() == a.data() && absent.get() == nullptr && packed.get() != a.data());
    for (size_t j = 0; j < pos.size(); ++j)
      for (long c = 0; c < w; ++c) CHECK(packed.get()[j * (size_t)w + (size_t)c] == a[(size_t)(pos[j] * w + c)]);
    te::RowsIn<double> nothing(a.data(), &none, w);   // (never read: a part without rows is not called)
    (void)nothing;
    std::vector<double> out((size_t)(n * w), -2.0);
    te::RowsOut<double> direct(out.data(), nullptr, w), buffered(out.data(), &pos, w), missing((double*)nullptr, &pos, w);
    CHECK(direct.get() == out.data() && missing.get() == nullptr && buffered.get() != out.data());
    for (size_t j = 0; j < pos.size() * (size_t)w; ++j) { CHECK(buffered.get()[j] == 0.0); buffered.get()[j] = 100.0 + (double)j; }
    direct.scatter();    // nothing to do
    missing.scatter();   // nowhere to write
    for (double v : out) CHECK(v == -2.0);
    buffered.scatter();
    for (long i = 0; i < n; ++i) {
      const auto it = std::find(pos.begin(), pos.end(), i);
      for (long c = 0; c < w; ++c)
        CHECK(out[(size_t)(i * w + c)] == (it == pos.end() ? -2.0 : 100.0 + (double)((it - pos.begin()) * w + c)));
    }
  }
  // new ids only: ids that exist and ids named twice in the call are left out and reported, in the caller's order
  const unsigned ids[8] = {4, 9, 4, 2, 7, 9, 11, 2};
  std::vector<unsigned> again;
  const std::vector<long> keep = te::newIdsOnly(ids, 8, [](unsigned id) { return id == 7; }, [&](unsigned id) { again.push_back(id); });
  CHECK(keep == std::vector<long>({0, 1, 3, 6}));
  CHECK(again == std::vector<unsigned>({4, 7, 9, 2}));
  CHECK(te::newIdsOnly(ids, 0, [](unsigned) { return false; }, [](unsigned) {}).empty());
  CHECK(te::newIdsOnly(nullptr, -3, [](unsigned) { return false; }, [](unsigned) {}).empty());
}

int main() {
  test_row_split();
  test_single_creations();
  test_batched_runs();
  test_erase_and_recreate();
  test_ranks();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("shard map tests ok\n");
  return 0;
}
