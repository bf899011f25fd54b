// dt_table_ring.hpp -- the device table of a fused call with a time-step schedule (kf_step_sep.hpp, DTTAB), owned by whoever
// launches the call: a Batch for its own fused calls, a Shard for the one launch that replays all of its batches.
// Every call takes a fresh run of a ring -- pinned host words the schedule is copied into before the call returns, and the device
// words behind them, filled by a copy on the owner's stream ahead of the launch -- so two calls enqueued back to back never share
// a word; the ring wraps, or grows, behind a synchronisation of the stream.  The device block goes through device_free (deferred
// while a resident session of the process is alive); retired host blocks are kept until the owner goes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "hip_check.hpp"

namespace te {

class DtTableRing {
 public:
  DtTableRing() = default;
  DtTableRing(const DtTableRing&) = delete;
  DtTableRing& operator=(const DtTableRing&) = delete;
  ~DtTableRing() {
    device_free(d_);
    if (h_) (void)hipHostFree(h_);
    for (double* h : retired_) (void)hipHostFree(h);
  }
  // the device address of the call's n entries, filled on `stream`
  const double* push(const double* dt_host, long n, hipStream_t stream) {
    if (n > cap_) {   // grow: nothing in flight may still read the old blocks
      const long want = (std::max<long>(std::max<long>(n, 256), cap_ * 2) + 15) / 16 * 16;
      TE_HIP_CHECK(hipStreamSynchronize(stream));
      double* h = nullptr;
      double* d = nullptr;
      TE_HIP_CHECK(hipHostMalloc((void**)&h, (size_t)want * sizeof(double), hipHostMallocDefault));
      if (hipMalloc((void**)&d, (size_t)want * sizeof(double)) != hipSuccess) {
        (void)hipHostFree(h);
        throw std::runtime_error("target_estimation_amd: no device memory for the time-step table");
      }
      device_free(d_);   // (deferred while a resident session of the process is alive)
      if (h_) retired_.push_back(h_);
      d_ = d; h_ = h; cap_ = want; off_ = 0;
    } else if (off_ + n > cap_) {   // wrap: the runs at the head of the ring may still be in flight
      TE_HIP_CHECK(hipStreamSynchronize(stream));
      off_ = 0;
    }
    double* h = h_ + off_;
    double* d = d_ + off_;
    std::memcpy(h, dt_host, (size_t)n * sizeof(double));   // (the caller's array is read here, before the call returns)
    TE_HIP_CHECK(hipMemcpyAsync(d, h, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream));
    off_ += n;
    return d;
  }

 private:
  double* d_ = nullptr;
  double* h_ = nullptr;
  long cap_ = 0, off_ = 0;
  std::vector<double*> retired_;
};

}  // namespace te
