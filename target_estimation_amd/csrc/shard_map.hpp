// shard_map.hpp -- the id -> shard map and the placement rule of a manager spread over several devices
// (target_manager_set_devices).  Host-only and HIP-free, so that g++ with ASan/UBSan tests it
// (tests/host/shard_map_test.cpp).
//
// Placement:
//   * a single creation goes to the shard that holds the fewest targets of its motion model; ties go to
//     the lowest shard index;
//   * a batched creation of k ids of one model is cut into contiguous runs, in the caller's order: the
//     water-filling of the per-model counts (the lowest shards are raised first, a remainder goes to the
//     lowest indices) decides how many ids each shard takes, and the runs are handed out in shard order.
//     The counts it reaches are those of k single creations in a row;
//   * an erased id that is created again is placed by the rule as it stands at that moment.
#pragma once

#include <algorithm>
#include <cstddef>
#include <unordered_map>
#include <utility>
#include <vector>

namespace te {

class ShardMap {
 public:
  static constexpr int kModels = 4;

  void reset(int n_shards) {
    n_ = n_shards;
    count_.assign((size_t)n_shards * kModels, 0);
    where_.clear();
  }
  int shards() const { return n_; }
  long count(int shard, int model) const { return count_[(size_t)shard * kModels + (size_t)model]; }

  // the shard of id, or -1
  int shard_of(unsigned id) const {
    auto it = where_.find(id);
    return it == where_.end() ? -1 : it->second.first;
  }
  bool contains(unsigned id) const { return where_.count(id) != 0; }
  size_t size() const { return where_.size(); }

  // where a single creation of `model` goes
  int place_one(int model) const {
    int best = 0;
    for (int s = 1; s < n_; ++s)
      if (count(s, model) < count(best, model)) best = s;
    return best;
  }

  // how many of k new ids of `model` each shard takes (water-filling towards equal per-model counts)
  std::vector<long> place_amounts(int model, long k) const {
    std::vector<long> add((size_t)n_, 0);
    long left = k;
    while (left > 0) {
      long low = -1;
      for (int s = 0; s < n_; ++s) {
        const long c = count(s, model) + add[(size_t)s];
        if (low < 0 || c < low) low = c;
      }
      std::vector<int> lows;
      long next = -1;   // the next level above `low`, -1: none
      for (int s = 0; s < n_; ++s) {
        const long c = count(s, model) + add[(size_t)s];
        if (c == low) lows.push_back(s);
        else if (next < 0 || c < next) next = c;
      }
      const long m = (long)lows.size();
      if (next >= 0 && (next - low) * m <= left) {
        for (int s : lows) add[(size_t)s] += next - low;
        left -= (next - low) * m;
      } else {
        const long q = left / m, r = left % m;
        for (long j = 0; j < m; ++j) add[(size_t)lows[(size_t)j]] += q + (j < r ? 1 : 0);
        left = 0;
      }
    }
    return add;
  }

  // shard of each of the k new ids (contiguous runs, shard 0's run first)
  std::vector<int> place_batch(int model, long k) const {
    const std::vector<long> add = place_amounts(model, k);
    std::vector<int> out;
    out.reserve((size_t)k);
    for (int s = 0; s < n_; ++s) out.insert(out.end(), (size_t)add[(size_t)s], s);
    return out;
  }

  void insert(unsigned id, int shard, int model) {
    where_[id] = std::make_pair(shard, model);
    ++count_[(size_t)shard * kModels + (size_t)model];
  }
  // false: unknown id
  bool erase(unsigned id) {
    auto it = where_.find(id);
    if (it == where_.end()) return false;
    --count_[(size_t)it->second.first * kModels + (size_t)it->second.second];
    where_.erase(it);
    return true;
  }

 private:
  int n_ = 0;
  std::vector<long> count_;                                   // [shard][model]
  std::unordered_map<unsigned, std::pair<int, int>> where_;   // id -> (shard, model)
};

// ascending merge of several ascending id lists (the shards' getAvailableTargets)
inline std::vector<unsigned> merge_sorted_ids(const std::vector<std::vector<unsigned>>& lists) {
  std::vector<unsigned> out;
  size_t total = 0;
  for (const auto& l : lists) total += l.size();
  out.reserve(total);
  std::vector<size_t> at(lists.size(), 0);
  for (;;) {
    int pick = -1;
    for (size_t k = 0; k < lists.size(); ++k)
      if (at[k] < lists[k].size() && (pick < 0 || lists[k][at[k]] < lists[(size_t)pick][at[(size_t)pick]])) pick = (int)k;
    if (pick < 0) break;
    out.push_back(lists[(size_t)pick][at[(size_t)pick]++]);
  }
  return out;
}

// rank_of_slot of one batch: the row of each slot's id in the ascending list of every id of the manager
// (sorted_all), -1 for an id that is not there
inline void ranks_of_slots(const std::vector<unsigned>& sorted_all, const unsigned* slot_ids, long n, int* rank_out) {
  for (long s = 0; s < n; ++s) {
    auto it = std::lower_bound(sorted_all.begin(), sorted_all.end(), slot_ids[s]);
    rank_out[s] = (it != sorted_all.end() && *it == slot_ids[s]) ? (int)(it - sorted_all.begin()) : -1;
  }
}

}  // namespace te
