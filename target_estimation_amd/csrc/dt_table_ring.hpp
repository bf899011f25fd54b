// dt_table_ring.hpp -- the device table of a fused call with a time-step schedule (kf_step_sep.hpp, DTTAB), owned by whoever
// launches the call: a Batch for its own fused calls, a Shard for the one launch that replays all of its batches.
// Every call takes a fresh run of a ring -- pinned host words the schedule is copied into before the call returns, and the device
// words behind them, filled by a copy on the owner's stream ahead of the launch -- so two calls enqueued back to back never share
// a word; the ring wraps, or grows, behind a synchronisation of the stream.  The device block goes through device_free (deferred
// while a resident session of the process is alive); retired host blocks are kept until the owner goes.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "dev_mem.hpp"

namespace te {

class DtTableRing {
 public:
  DtTableRing() = default;
  DtTableRing(const DtTableRing&) = delete;
  DtTableRing& operator=(const DtTableRing&) = delete;
  // the device address of the call's n entries, filled on `stream`
  const double* push(const double* dt_host, long n, hipStream_t stream) {
    if (n > cap_) {   // grow: nothing in flight may still read the old blocks
      const long want = (std::max<long>(std::max<long>(n, 256), cap_ * 2) + 15) / 16 * 16;
      dev_mem_check(hipStreamSynchronize(stream), "DtTableRing::push: hipStreamSynchronize");
      PinnedBuf<double> h;
      DeviceBuf<double> d;
      h.alloc((size_t)want);
      if (!d.try_alloc((size_t)want)) throw std::runtime_error("target_estimation_amd: no device memory for the time-step table");
      if (h_) retired_.push_back(std::move(h_));
      d_ = std::move(d);   // (the old block's free is deferred while a resident session of the process is alive)
      h_ = std::move(h); cap_ = want; off_ = 0;
    } else if (off_ + n > cap_) {   // wrap: the runs at the head of the ring may still be in flight
      dev_mem_check(hipStreamSynchronize(stream), "DtTableRing::push: hipStreamSynchronize");
      off_ = 0;
    }
    double* h = h_.host() + off_;
    double* d = d_.get() + off_;
    std::memcpy(h, dt_host, (size_t)n * sizeof(double));   // (the caller's array is read here, before the call returns)
    dev_mem_check(hipMemcpyAsync(d, h, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream), "DtTableRing::push: hipMemcpyAsync");
    off_ += n;
    return d;
  }

 private:
  long cap_ = 0, off_ = 0;
  std::vector<PinnedBuf<double>> retired_;
  PinnedBuf<double> h_;
  DeviceBuf<double> d_;
};

}  // namespace te
