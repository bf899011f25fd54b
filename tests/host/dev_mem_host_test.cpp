// dev_mem_host_test.cpp -- host checks of csrc/dev_mem.hpp (the owning types of device buffers, pinned blocks, streams and events)
// and of csrc/dt_table_ring.hpp on top of them, against malloc-backed fakes of the few runtime functions the headers call: every
// allocation and handle is counted per kind, the k-th allocation can be told to fail.  Not linked against the HIP runtime.  Built
// with g++ -fsanitize=address,undefined by tests/test_dev_mem_host.py.  Prints "dev mem host test ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../target_estimation_amd/csrc/dev_mem.hpp"
#include "../../target_estimation_amd/csrc/dt_table_ring.hpp"

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
  } while (0)

// ---------------------------------------------------------------- the fakes
namespace fake {
std::set<void*> device, pinned, streams, events;   // what is live, by kind
long device_free_calls = 0;   // releases of non-null device memory through te::device_free
long hip_free_calls = 0;      // ... through hipFree directly: never
long double_release = 0;      // a release of something that is not live
int fail_in = 0;              // > 0: the fail_in-th allocation from now on fails (device and pinned memory count together)
hipError_t last_error = hipSuccess;

bool fails() { return fail_in > 0 && --fail_in == 0; }
hipError_t allocate(std::set<void*>& kind, void** p, size_t bytes) {
  if (fails()) { *p = nullptr; return last_error = hipErrorOutOfMemory; }
  *p = std::malloc(bytes ? bytes : 1);
  kind.insert(*p);
  return hipSuccess;
}
void release(std::set<void*>& kind, void* p) {
  if (kind.erase(p) != 1) { ++double_release; return; }
  std::free(p);
}
template <class H>
hipError_t create(std::set<void*>& kind, H* h) {
  void* p = nullptr;
  allocate(kind, &p, 1);
  *h = reinterpret_cast<H>(p);
  return hipSuccess;
}
bool all_released() { return device.empty() && pinned.empty() && streams.empty() && events.empty(); }
}  // namespace fake

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake::allocate(fake::device, p, bytes); }
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned) { return fake::allocate(fake::device, p, bytes); }
hipError_t hipFree(void* p) { ++fake::hip_free_calls; fake::release(fake::device, p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake::allocate(fake::pinned, p, bytes); }
hipError_t hipHostFree(void* p) { fake::release(fake::pinned, p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake::create(fake::streams, s); }
hipError_t hipStreamDestroy(hipStream_t s) { fake::release(fake::streams, s); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake::create(fake::events, e); }
hipError_t hipEventDestroy(hipEvent_t e) { fake::release(fake::events, e); return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { std::memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError(void) { const hipError_t e = fake::last_error; fake::last_error = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake error"; }
}

namespace te {
void device_free(void* p) {   // (the library's defers the release while a resident session is alive; the fake releases at once)
  if (!p) return;
  ++fake::device_free_calls;
  fake::release(fake::device, p);
}
}  // namespace te

using te::DeviceBuf;
using te::PinnedBuf;

template <class Owner, class Alloc>
static void check_owner(std::set<void*>& kind, Alloc alloc) {
  const size_t before = kind.size();
  {   // a moved-from owner is empty, and the target releases exactly once
    Owner a;
    alloc(a);
    CHECK(a && kind.size() == before + 1);
    Owner b(std::move(a));
    CHECK(!a && b && kind.size() == before + 1);
  }
  CHECK(kind.size() == before);
  {   // move-assignment over a live owner releases the old block once
    Owner a, b;
    alloc(a); alloc(b);
    CHECK(kind.size() == before + 2);
    a = std::move(b);
    CHECK(a && !b && kind.size() == before + 1);
  }
  CHECK(kind.size() == before);
  {   // self-move and swap are safe; reset() is idempotent
    Owner a, b;
    alloc(a);
    Owner& self = a;
    a = std::move(self);
    CHECK(a && kind.size() == before + 1);
    a.swap(b);
    CHECK(!a && b && kind.size() == before + 1);
    a.swap(a); b.swap(b);
    CHECK(!a && b);
    b.reset(); b.reset(); a.reset();
    CHECK(!a && !b && kind.size() == before);
  }
  CHECK(fake::double_release == 0);
}

static void test_device_buf() {
  check_owner<DeviceBuf<double>>(fake::device, [](DeviceBuf<double>& b) { b.alloc(8); });
  check_owner<DeviceBuf<char>>(fake::device, [](DeviceBuf<char>& b) { CHECK(b.try_alloc_finegrained(128)); });
  {   // the elements are T's
    DeviceBuf<double> b;
    b.alloc(5);
    for (int i = 0; i < 5; ++i) b.get()[i] = i;   // (the sanitizer objects if the block is short)
    CHECK(b.get()[4] == 4.0);
  }
  {   // try_alloc that fails: empty, nothing thrown, the runtime's last error clear -- over a live block too
    DeviceBuf<int> b;
    fake::fail_in = 1;
    CHECK(!b.try_alloc(4) && !b && b.get() == nullptr);
    CHECK(hipGetLastError() == hipSuccess);
    CHECK(b.try_alloc(4) && b);
    fake::fail_in = 1;
    CHECK(!b.try_alloc(8) && !b && fake::device.empty());
    CHECK(hipGetLastError() == hipSuccess);
    fake::fail_in = 1;
    CHECK(!b.try_alloc_finegrained(8) && !b);
    CHECK(hipGetLastError() == hipSuccess);
  }
  {   // alloc that fails: throws, empty, last error clear
    DeviceBuf<int> b;
    b.alloc(4);
    fake::fail_in = 1;
    bool thrown = false;
    try { b.alloc(8); } catch (const std::runtime_error& e) { thrown = std::strstr(e.what(), "HIP error") != nullptr; }
    CHECK(thrown && !b && fake::device.empty());
    CHECK(hipGetLastError() == hipSuccess);
  }
  // device buffers go through te::device_free, never through hipFree
  CHECK(fake::device_free_calls > 0 && fake::hip_free_calls == 0);
}

static void test_pinned_buf() {
  check_owner<PinnedBuf<int>>(fake::pinned, [](PinnedBuf<int>& b) { b.alloc(16); });
  check_owner<PinnedBuf<char>>(fake::pinned, [](PinnedBuf<char>& b) { b.alloc(64, te::kPinnedMapped); });
  const long device_frees = fake::device_free_calls;
  {
    PinnedBuf<char> plain, mapped;
    plain.alloc(32);
    mapped.alloc(32, te::kPinnedMapped);
    CHECK(plain.host() && plain.dev() == nullptr);          // no device alias unless the block is mapped
    CHECK(mapped.host() && mapped.dev() == mapped.host());  // (the fake maps a block onto itself)
    PinnedBuf<char> moved(std::move(mapped));
    CHECK(moved.dev() == moved.host() && mapped.dev() == nullptr && mapped.host() == nullptr);
    fake::fail_in = 1;
    bool thrown = false;
    try { plain.alloc(64); } catch (const std::runtime_error&) { thrown = true; }
    CHECK(thrown && !plain && plain.host() == nullptr);
    CHECK(hipGetLastError() == hipSuccess);
    CHECK(fake::pinned.size() == 1);
  }
  // pinned blocks are released with hipHostFree: neither of the device paths saw them
  CHECK(fake::pinned.empty() && fake::device_free_calls == device_frees && fake::hip_free_calls == 0);
}

static void test_handles() {
  check_owner<te::Stream>(fake::streams, [](te::Stream& s) { hipStreamCreateWithFlags(s.out(), 0); });
  check_owner<te::Event>(fake::events, [](te::Event& e) { hipEventCreateWithFlags(e.out(), 0); });
  te::Stream s;
  hipStreamCreateWithFlags(s.out(), 0);
  const hipStream_t first = s.get();
  hipStreamCreateWithFlags(s.out(), 0);   // out() over a live handle destroys it first
  CHECK(fake::streams.size() == 1 && fake::streams.count(first) == 0);
}

static void test_dt_table_ring() {
  std::vector<double> dt(2000);
  for (size_t i = 0; i < dt.size(); ++i) dt[i] = 0.001 * (double)(i + 1);
  auto holds = [&](const double* d, long n) { return std::memcmp(d, dt.data(), (size_t)n * sizeof(double)) == 0; };
  {
    te::DtTableRing ring;
    const double* a = ring.push(dt.data(), 100, nullptr);   // grow: 0 -> 256
    const double* b = ring.push(dt.data(), 100, nullptr);
    CHECK(b == a + 100 && holds(a, 100) && holds(b, 100));
    const double* c = ring.push(dt.data(), 100, nullptr);   // wrap
    CHECK(c == a && fake::device.size() == 1 && fake::pinned.size() == 1);
    const double* d = ring.push(dt.data(), 600, nullptr);   // grow again: the host block is retired, the device block released
    CHECK(holds(d, 600) && fake::device.size() == 1 && fake::pinned.size() == 2 && fake::device.count((void*)a) == 0);
    const double* e = ring.push(dt.data(), 8, nullptr);     // (600 rounds up to 608 entries)
    CHECK(e == d + 600);
    // the device allocation of a growth fails (the second allocation: the pinned block comes first): the new host block is
    // released, the ring is as it was
    fake::fail_in = 2;
    bool thrown = false;
    try { ring.push(dt.data(), 2000, nullptr); } catch (const std::runtime_error&) { thrown = true; }
    CHECK(thrown && hipGetLastError() == hipSuccess);
    CHECK(fake::device.size() == 1 && fake::pinned.size() == 2 && fake::device.count((void*)d) == 1);
    const double* f = ring.push(dt.data(), 600, nullptr);   // a push of the old size is still served, from the block owned before
    CHECK(f == d && holds(f, 600) && holds(e, 8));   // (wrapped; the addresses returned before are still the ring's)
    // ... and a failure of the pinned allocation leaves it usable as well
    fake::fail_in = 1;
    thrown = false;
    try { ring.push(dt.data(), 2000, nullptr); } catch (const std::runtime_error&) { thrown = true; }
    CHECK(thrown && fake::device.size() == 1 && fake::pinned.size() == 2);
    CHECK(ring.push(dt.data(), 2000, nullptr) != nullptr && fake::device.size() == 1 && fake::pinned.size() == 3);
  }
  CHECK(fake::all_released());   // the ring, its retired host blocks included, is gone
}

int main() {
  test_device_buf();
  CHECK(fake::all_released());
  test_pinned_buf();
  CHECK(fake::all_released());
  test_handles();
  CHECK(fake::all_released());
  test_dt_table_ring();
  // every kind's live count is 0 at exit (asserted here, not left to the leak checker), nothing was released twice, hipFree never ran
  CHECK(fake::all_released() && fake::double_release == 0 && fake::hip_free_calls == 0);
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("dev mem host test ok\n");
  return 0;
}
