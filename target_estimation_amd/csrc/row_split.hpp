// row_split.hpp -- the gather -> call -> scatter of a host-array call whose rows belong to several parts: the manager splits
// the caller's ids by shard, a shard splits its ids by batch.  Either level records the POSITIONS of a part's rows in the
// caller's arrays (in the caller's order), hands the part packed copies of those rows and writes packed results back at the
// same positions.  A part that takes every row in order gets the caller's arrays themselves (pos == null): no copy.
// Host-only and HIP-free, so that g++ with ASan/UBSan tests it (tests/host/shard_map_test.cpp).
#pragma once

#include <cstddef>
#include <vector>

#include "id_table.hpp"

namespace te {

// positions into the caller's arrays per part, in the caller's order; the positions that belong to no part in `unknown`
struct Split {
  std::vector<std::vector<long>> src;
  std::vector<long> unknown;
};

// rows of width w of the caller's array at positions pos, packed (empty for a null array) / packed rows back at pos
template <class T>
std::vector<T> gatherRows(const T* a, const std::vector<long>& pos, long w) {
  std::vector<T> out;
  if (!a) return out;
  out.resize(pos.size() * (size_t)w);
  for (size_t j = 0; j < pos.size(); ++j)
    for (long c = 0; c < w; ++c) out[j * (size_t)w + (size_t)c] = a[pos[j] * w + c];
  return out;
}
template <class T>
void scatterRows(T* a, const std::vector<T>& rows, const std::vector<long>& pos, long w) {
  if (!a) return;
  for (size_t j = 0; j < pos.size(); ++j)
    for (long c = 0; c < w; ++c) a[pos[j] * w + c] = rows[j * (size_t)w + (size_t)c];
}

// An input array as one part sees it: the caller's array itself (pos == null), else a packed copy of its rows at *pos.
// A null array stays null.
template <class T>
class RowsIn {
 public:
  RowsIn(const T* a, const std::vector<long>* pos, long w) : p_(a) {
    if (a && pos) { buf_ = gatherRows(a, *pos, w); p_ = buf_.data(); }
  }
  const T* get() const { return p_; }

 private:
  const T* p_;
  std::vector<T> buf_;
};

// An output array as one part sees it: the caller's array itself (pos == null), else a zero-filled packed buffer whose rows
// scatter() writes to the caller's array at *pos.  A null array stays null.
template <class T>
class RowsOut {
 public:
  RowsOut(T* a, const std::vector<long>* pos, long w) : a_(a), pos_(pos), w_(w), p_(a) {
    if (a && pos) { buf_.assign(pos->size() * (size_t)w, T()); p_ = buf_.data(); }
  }
  T* get() { return p_; }
  void scatter() { if (a_ && pos_) scatterRows(a_, buf_, *pos_, w_); }

 private:
  T* a_;
  const std::vector<long>* pos_;
  long w_;
  T* p_;
  std::vector<T> buf_;
};

template <class... Outs>
void scatterAll(Outs&... outs) { (outs.scatter(), ...); }

// positions of the ids of a creation call that do not exist yet and were not named earlier in the same call (existing ones
// are left untouched, as in init()); exists(id) asks the table of whoever creates, again(id) is told every id left out
template <class Exists, class Again>
std::vector<long> newIdsOnly(const unsigned* ids, long n, Exists&& exists, Again&& again) {
  std::vector<long> keep;
  keep.reserve((size_t)(n > 0 ? n : 0));
  IdTable seen;
  seen.reserve((size_t)(n > 0 ? n : 0));
  for (long i = 0; i < n; ++i) {
    if (exists(ids[i]) || seen.contains(ids[i])) { again(ids[i]); continue; }
    seen.set(ids[i], TargetLoc{0, 0});
    keep.push_back(i);
  }
  return keep;
}

}  // namespace te
