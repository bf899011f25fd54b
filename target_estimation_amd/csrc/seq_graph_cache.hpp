// seq_graph_cache.hpp -- the recorded launch sequences of one owner (Batch::step_sequence, Shard::stepSequenceAll): hipGraph_t /
// hipGraphExec_t pairs filed under the owner's key type, at most `capacity` of them.  The protocol both owners follow:
//   find(pred)                    the recording whose key satisfies pred, or null
//   record(key, running, cap, f)  make room -- the recording with the smallest stamp goes, behind a synchronisation of `running`,
//                                 the stream it may still be replaying on --, capture f() on `cap`, instantiate, file under key
//   stamp(e)                      e is the newest from now on
// A new recording is stamped.  An owner that stamps every use as well evicts the least recently used recording; one that never
// stamps evicts the oldest.  A failure of f() or of the instantiation leaves neither a stream in capture mode nor a graph behind.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <utility>
#include <vector>

#include "dev_mem.hpp"
#include "hip_check.hpp"

namespace te {

template <class Key>
class SeqGraphCache {
 public:
  struct Entry {
    Key key;
    Graph graph;
    GraphExec exec;   // (declared behind the graph: destroyed before it)
    unsigned long stamp = 0;
  };

  explicit SeqGraphCache(size_t capacity) : capacity_(capacity) {}
  ~SeqGraphCache() { drop(); }
  SeqGraphCache(const SeqGraphCache&) = delete;
  SeqGraphCache& operator=(const SeqGraphCache&) = delete;

  template <class Pred>
  Entry* find(Pred&& pred) {
    for (auto& e : entries_)
      if (pred(e.key)) return &e;
    return nullptr;
  }
  void stamp(Entry& e) { e.stamp = ++clock_; }
  long recordings() const { return recordings_; }   // recordings made so far
  void drop() { entries_.clear(); }                 // (the owner knows that none is running)

  // The returned entry stays where it is until the next record() or drop().
  template <class Body>
  Entry& record(Key key, hipStream_t running, hipStream_t capture, Body&& body) {
    if (entries_.size() >= capacity_) {
      size_t victim = 0;
      for (size_t k = 1; k < entries_.size(); ++k)
        if (entries_[k].stamp < entries_[victim].stamp) victim = k;
      TE_HIP_CHECK(hipStreamSynchronize(running));   // it may still be running
      entries_.erase(entries_.begin() + (long)victim);
    }
    Entry e{std::move(key)};
    TE_HIP_CHECK(hipStreamBeginCapture(capture, hipStreamCaptureModeThreadLocal));
    try {
      body();
    } catch (...) {
      (void)hipStreamEndCapture(capture, e.graph.out());   // never leave the stream in capture mode
      throw;
    }
    TE_HIP_CHECK(hipStreamEndCapture(capture, e.graph.out()));
    if (hipGraphInstantiate(e.exec.out(), e.graph.get(), nullptr, nullptr, 0) != hipSuccess)
      throw std::runtime_error("target_estimation_amd: hipGraphInstantiate failed for a step sequence");
    stamp(e);
    entries_.push_back(std::move(e));
    ++recordings_;
    return entries_.back();
  }

 private:
  const size_t capacity_;
  std::vector<Entry> entries_;
  unsigned long clock_ = 0;
  long recordings_ = 0;
};

}  // namespace te
