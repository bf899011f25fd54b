// zigzag_ceiling.hip -- does alternating the traversal direction between ticks keep the tail of the state in the
// 256 MB Infinity Cache?  The step kernels' tile pattern (AoSoA lane records, in place or ping-pong), tick s walking
// the tiles forwards and tick s+1 backwards ("zig-zag"), against forwards every tick.
// "per-XCD": the backward tick mirrors the blocks inside each residue class mod 8 (csrc/zigzag_map.hpp) instead of over
// the whole grid, so a tile is stepped by a block of the same class -- by observation the same XCD, hence the same L2 --
// in both directions.  "rotated" is its control: the same order of addresses, every tile on a neighbouring class.
// `meas`: every lane also reads 56 bytes of a read-only stream, as the step kernels read their measurements.
// The last lines print HW_REG_XCC_ID of some blocks over consecutive launches on one stream: the premise of
// "per-XCD" is that block b of consecutive launches lands on the same XCD, which is observed behaviour and no contract.
// build: hipcc --offload-arch=gfx950 -O3 tools/zigzag_ceiling.hip -o tools/_build/zigzag_ceiling
// run:   tools/_build/zigzag_ceiling [rounds]      (every figure is printed `rounds` times, default 3: the spread)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "../target_estimation_amd/csrc/zigzag_map.hpp"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

// reverse: 0 forwards, 1 mirror over the grid's tiles, 2 mirror per class of blocks (te::zz_block), 3 the control: the order of 2 with
// every whole group of 8 blocks rotated by one class, i.e. the same address order on the wrong XCDs
template <int NCH, bool NT, bool MEAS, bool PROBE>
__global__ void __launch_bounds__(256) tile_kernel(const v4f* in, v4f* out, const v2f* meas, long n_tiles, int reverse, int* xcc) {
  const int lane = threadIdx.x & 63;
  unsigned b = blockIdx.x;
  if constexpr (PROBE) {
    if (threadIdx.x == 0) {
      unsigned id;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(id));
      xcc[b] = (int)id;
    }
  }
  if (reverse >= 2) b = te::zz_block(b, gridDim.x);
  if (reverse == 3 && (b | 7u) < gridDim.x) b = (b & ~7u) | ((b + 1) & 7u);
  long tile = (long)b * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;
  if (reverse == 1) tile = n_tiles - 1 - tile;
  const v4f* ti = in + tile * (long)NCH * 64;
  v4f* to = out + tile * (long)NCH * 64;
  v4f r[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) r[c] = ti[c * 64 + lane];
  if constexpr (MEAS) {   // 7 rows of 8 bytes per lane = 56 bytes, SoA rows inside the tile like the state
    const v2f* tm = meas + tile * 7L * 64;
#pragma unroll
    for (int c = 0; c < 7; ++c) r[c % NCH].y += tm[c * 64 + lane].x;
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    r[c].x += 1.0f;
    if constexpr (NT) __builtin_nontemporal_store(r[c], &to[c * 64 + lane]);
    else to[c * 64 + lane] = r[c];
  }
}

template <int NCH, bool MEAS>
void run(long n_targets, int rounds) {
  const long n_tiles = (n_targets + 63) / 64;
  const size_t bytes = (size_t)n_tiles * NCH * 64 * 16, mbytes = (size_t)n_tiles * 7 * 64 * 8;
  v4f *a, *b;
  v2f* m = nullptr;
  (void)hipMalloc(&a, bytes); (void)hipMalloc(&b, bytes);
  (void)hipMemset(a, 0, bytes); (void)hipMemset(b, 0, bytes);
  if (MEAS) { (void)hipMalloc(&m, mbytes); (void)hipMemset(m, 0, mbytes); }
  const int NM = 8;
  const char* names[NM] = {"in place, forwards   ", "in place, zig-zag    ", "in place, zz per-XCD ", "in place, zz rotated ", "ping-pong, forwards  ",
                           "ping-pong, zig-zag   ", "ping-pong nt, fwd    ", "ping-pong nt, zig-zag"};
  const int dir[NM] = {0, 1, 2, 3, 0, 1, 0, 1};
  const unsigned tb = (unsigned)((n_tiles + 3) / 4);
  for (int round = 0; round < rounds; ++round)
    for (int mode = 0; mode < NM; ++mode) {
      const bool pp = mode >= 4, nt = mode >= 6;
      hipEvent_t e0, e1;
      (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
      const int reps = 20;
      for (int r = 0; r < reps + 4; ++r) {
        if (r == 4) (void)hipEventRecord(e0, 0);
        const int rev = (r & 1) ? dir[mode] : 0;
        v4f* out = pp ? b : a;
        if (nt) hipLaunchKernelGGL((tile_kernel<NCH, true, MEAS, false>), dim3(tb), dim3(256), 0, 0, a, out, m, n_tiles, rev, nullptr);
        else hipLaunchKernelGGL((tile_kernel<NCH, false, MEAS, false>), dim3(tb), dim3(256), 0, 0, a, out, m, n_tiles, rev, nullptr);
        if (pp) std::swap(a, b);
      }
      (void)hipEventRecord(e1, 0);
      (void)hipEventSynchronize(e1);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0, e1);
      (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
      ms /= reps;
      printf("targets %9ld  %4d B/lane%s  state %6.0f MB  round %d  %s %8.1f us  %6.0f GB/s\n", n_targets, NCH * 16, MEAS ? " + 56 B read" : "", bytes / 1e6,
             round, names[mode], ms * 1e3, (2.0 * bytes + (MEAS ? mbytes : 0)) / (ms * 1e-3) / 1e9);
    }
  (void)hipFree(a); (void)hipFree(b);
  if (m) (void)hipFree(m);
}

// Where do the blocks of consecutive launches land?  The in-place per-XCD zig-zag at 240 MB, every block noting its XCD.
void probe() {
  constexpr int NCH = 15, LAUNCHES = 8;
  const long n_tiles = (1000000 + 63) / 64;
  const size_t bytes = (size_t)n_tiles * NCH * 64 * 16;
  const unsigned tb = (unsigned)((n_tiles + 3) / 4);
  v4f* a;
  int* xcc;
  (void)hipMalloc(&a, bytes); (void)hipMemset(a, 0, bytes);
  (void)hipMalloc(&xcc, sizeof(int) * tb * LAUNCHES); (void)hipMemset(xcc, 0xff, sizeof(int) * tb * LAUNCHES);
  for (int l = 0; l < LAUNCHES; ++l)
    hipLaunchKernelGGL((tile_kernel<NCH, false, false, true>), dim3(tb), dim3(256), 0, 0, a, a, nullptr, n_tiles, (l & 1) ? 2 : 0, xcc + (size_t)l * tb);
  (void)hipDeviceSynchronize();
  std::vector<int> h((size_t)tb * LAUNCHES);
  (void)hipMemcpy(h.data(), xcc, sizeof(int) * h.size(), hipMemcpyDeviceToHost);
  printf("HW_REG_XCC_ID over %d consecutive launches of %u blocks on one stream\n", LAUNCHES, tb);
  for (int l = 0; l < LAUNCHES; ++l) {
    const int* x = h.data() + (size_t)l * tb;
    long rr = 0, same = 0;
    for (unsigned i = 0; i < tb; ++i) {
      rr += x[i] == (int)((x[0] + i) % 8);
      same += x[i] == h[i];
    }
    printf("launch %d  block 0 -> %d  block 1 -> %d  block 8 -> %d  block %u -> %d   blocks on XCD (xcc[0] + b) %% 8: %ld of %u   on the XCD of launch 0: %ld of %u\n", l,
           x[0], x[1], x[8], tb - 1, x[tb - 1], rr, tb, same, tb);
  }
  (void)hipFree(a); (void)hipFree(xcc);
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 3;
  run<15, false>(1000000, rounds);   // 240 MB
  run<22, false>(1000000, rounds);   // 352 MB
  run<30, false>(1000000, rounds);   // 480 MB
  run<15, true>(1000000, rounds);
  run<22, true>(1000000, rounds);
  run<30, true>(1000000, rounds);
  run<15, false>(4000000, 1);   // 0.96 GB
  run<30, false>(4000000, 1);   // 1.9 GB
  probe();
  return 0;
}
