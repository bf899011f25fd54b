// dev_mem.hpp -- the owning types of the host layer: a pointer (or handle) plus its release, nothing else.
//   DeviceBuf<T>  device memory.  Released through te::device_free, which defers the free while a resident session of the
//                 process is alive (hip_check.hpp): the one place that rule lives.
//   PinnedBuf<T>  pinned host memory (hipHostMalloc with the flags given), with its device alias where the block is mapped.
//   Handle<..>    a runtime handle with its destroy function: Stream, Event, Graph, GraphExec.
// All are move-only.  alloc() releases what the owner holds FIRST (the staging blocks must never exist twice) and leaves the
// owner empty when it fails; growth that carries contents over allocates into local owners and commits by move or swap.
// Needs only the runtime API header: compiles as plain host code.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <stdexcept>
#include <string>
#include <utility>

namespace te {

void device_free(void* p);   // batch_store.cpp (see hip_check.hpp)

// throws what TE_HIP_CHECK throws, with the runtime's last error cleared; `what` names the call and, outside this header, the
// caller (this header cannot use the macro: it needs hip_check.hpp's full runtime header)
inline void dev_mem_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return;
  (void)hipGetLastError();
  throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e) + " (" + what + ")");
}

template <class T>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
    return *this;
  }
  ~DeviceBuf() { reset(); }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { device_free(std::exchange(p_, nullptr)); }
  void swap(DeviceBuf& o) noexcept { std::swap(p_, o.p_); }
  // count elements of T; false (owner empty, last error clear) if the device has no room
  bool try_alloc(size_t count) { return cleared(take(count, false)); }
  // ... in fine-grained device memory (what the host may write through the PCIe BAR)
  bool try_alloc_finegrained(size_t count) { return cleared(take(count, true)); }
  void alloc(size_t count) { dev_mem_check(take(count, false), "hipMalloc"); }

 private:
  hipError_t take(size_t count, bool finegrained) {
    reset();
    void* p = nullptr;
    const hipError_t e = finegrained ? hipExtMallocWithFlags(&p, count * sizeof(T), hipDeviceMallocFinegrained) : hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess) p_ = static_cast<T*>(p);
    return e;
  }
  static bool cleared(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
  }
  T* p_ = nullptr;
};

template <class T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); d_ = std::exchange(o.d_, nullptr); }
    return *this;
  }
  ~PinnedBuf() { reset(); }
  T* host() const { return h_; }
  T* dev() const { return d_; }   // the block as the device sees it (mapped blocks only), obtained once at allocation
  explicit operator bool() const { return h_ != nullptr; }
  void reset() {
    if (h_) (void)hipHostFree(h_);
    h_ = d_ = nullptr;
  }
  void swap(PinnedBuf& o) noexcept { std::swap(h_, o.h_); std::swap(d_, o.d_); }
  void alloc(size_t count, unsigned flags = hipHostMallocDefault) {
    reset();
    void* h = nullptr;
    dev_mem_check(hipHostMalloc(&h, count * sizeof(T), flags), "hipHostMalloc");
    h_ = static_cast<T*>(h);
    if (flags & hipHostMallocMapped) {
      void* d = nullptr;
      const hipError_t e = hipHostGetDevicePointer(&d, h, 0);
      if (e != hipSuccess) reset();
      dev_mem_check(e, "hipHostGetDevicePointer");
      d_ = static_cast<T*>(d);
    }
  }

 private:
  T* h_ = nullptr;
  T* d_ = nullptr;
};
constexpr unsigned kPinnedMapped = hipHostMallocMapped | hipHostMallocCoherent;

// A runtime handle and its destroy function.  out(): the (emptied) slot a create call fills, e.g.
//   TE_HIP_CHECK(hipStreamCreateWithFlags(s.out(), hipStreamNonBlocking));
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
    return *this;
  }
  ~Handle() { reset(); }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
  H* out() { reset(); return &h_; }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  void swap(Handle& o) noexcept { std::swap(h_, o.h_); }

 private:
  H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Graph = Handle<hipGraph_t, hipGraphDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

}  // namespace te
