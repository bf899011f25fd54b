// track_lifecycle.cpp -- a tracker whose population changes, from plain C++ (no Python, no torch): objects appear and vanish, the
// detector delivers unlabelled frames, and the tracker starts EMPTY.  Every frame: the detections are paired with the targets on
// the device (target_manager_associate_grid_dev), one tick consumes the result (target_manager_step_sequence_all, n_ticks = 1), and
// target_manager_lifecycle turns every unmatched detection into a new target and retires every target that went K frames without a
// match -- only the counts, the retired ids and the new id range come back to the host.
// What it replaces: reading the unmatched rows back, a miss counter per id on the host, init_batch and erase_batch.
//   hipcc --offload-arch=gfx950 -O2 -I include/target_estimation_amd examples/track_lifecycle.cpp -o track_lifecycle \
//         -L target_estimation_amd/lib -ltarget_estimation_amd -Wl,-rpath,$PWD/target_estimation_amd/lib
//   ./track_lifecycle models 2000 8        (objects, frames)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "target_batch_c.h"
#include "target_manager_c.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "models";
  const long n = argc > 2 ? std::atol(argv[2]) : 2000;
  const long frames = argc > 3 ? std::atol(argv[3]) : 8;
  if (n < 1 || n > 1000000 || frames < 1) { std::fprintf(stderr, "usage: %s models n frames (n <= 1000000)\n", argv[0]); return 1; }
  const double dt = 0.004, noise = 0.001, gate = 9.0, cell = 2.0;
  const int rounds = 4, K = 2;
  target_manager_c* m = target_manager_new_ex((dir + "/model_uniform_velocity_params.yaml").c_str(), TARGET_DTYPE_F64, 0);
  if (!m) return 3;
  hipStream_t stream;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  target_manager_set_stream(m, stream);
  // the world: object i rests on a lattice of 4 m and is there from frame first[i] up to, not including, frame last[i]
  std::mt19937_64 rng(2026);
  std::normal_distribution<double> gauss(0.0, noise);
  std::vector<long> first((size_t)n), last((size_t)n);
  for (long i = 0; i < n; ++i) {
    first[(size_t)i] = (long)(rng() % (unsigned long)frames);
    last[(size_t)i] = first[(size_t)i] + 1 + (long)(rng() % (unsigned long)frames);
  }
  double *det_dev = nullptr, *meas_dev = nullptr;
  unsigned char* has_dev = nullptr;
  int *slot_of_det_dev = nullptr, *info_dev = nullptr;
  HIP_OK(hipMalloc((void**)&det_dev, sizeof(double) * 7 * n)); HIP_OK(hipMalloc((void**)&meas_dev, sizeof(double) * 7 * n));
  HIP_OK(hipMalloc((void**)&has_dev, (size_t)n)); HIP_OK(hipMalloc((void**)&slot_of_det_dev, sizeof(int) * n));
  HIP_OK(hipMalloc((void**)&info_dev, sizeof(int) * 4));
  target_assoc_out_c per;
  std::memset(&per, 0, sizeof per);
  per.meas_out_dev = meas_dev; per.ld = n; per.has_meas_out_dev = has_dev;
  target_batch_sequence_c seq;
  std::memset(&seq, 0, sizeof seq);
  seq.meas_dev = meas_dev; seq.tick_stride = 7 * n; seq.ld = n; seq.has_meas_dev = has_dev; seq.has_stride = n;
  const unsigned char* masks[1] = {has_dev};
  target_lifecycle_c policy;
  std::memset(&policy, 0, sizeof policy);
  policy.max_misses = K;                          // gone after K frames without a match
  policy.birth_type = TARGET_UNIFORM_VELOCITY;    // the model file's parameters (Q = R = P0 = NULL)
  policy.max_births = n;
  policy.dt0 = dt;
  std::vector<unsigned> retired((size_t)n);
  std::vector<double> frame;
  unsigned next_id = 1;
  bool ok = true;
  for (long f = 0; f < frames; ++f) {
    // the frame: every object that is there, in a random order
    std::vector<long> order;
    for (long i = 0; i < n; ++i) if (first[(size_t)i] <= f && f < last[(size_t)i]) order.push_back(i);
    std::shuffle(order.begin(), order.end(), rng);
    const long M = (long)order.size();
    frame.assign((size_t)M * 7, 0.0);
    for (long j = 0; j < M; ++j) {
      const long i = order[(size_t)j];
      double* d = &frame[(size_t)j * 7];
      d[0] = 4.0 * (double)(i % 64) + gauss(rng); d[1] = 4.0 * (double)((i / 64) % 64) + gauss(rng); d[2] = 4.0 * (double)(i / 4096) + gauss(rng);
      d[6] = 1.0;
    }
    if (M > 0) HIP_OK(hipMemcpyAsync(det_dev, frame.data(), sizeof(double) * 7 * M, hipMemcpyHostToDevice, stream));
    const int nb = target_manager_num_batches(m);   // 0 until the first births
    // pair on the device ...
    if (target_manager_associate_grid_dev(m, dt, det_dev, M, gate, rounds, cell, &per, nb, slot_of_det_dev, nullptr, nullptr, info_dev) != 0) {
      std::fprintf(stderr, "associate: %s\n", target_manager_last_error());
      return 5;
    }
    // ... one tick consumes the pairing ...
    if (nb > 0 && target_manager_step_sequence_all(m, 1, dt, &seq, nb, 0, nullptr, 0.0, 0) != 0) {
      std::fprintf(stderr, "step: %s\n", target_manager_last_error());
      return 6;
    }
    // ... and the population follows the frame.  (The masks and measurements above are stale from here on: slots move.)
    policy.first_id = next_id;
    policy.t_birth = dt * (double)(f + 1);
    long info[6];
    if (target_manager_lifecycle(m, det_dev, slot_of_det_dev, M, masks, nb, &policy, retired.data(), n, info) != 0) {
      std::fprintf(stderr, "lifecycle: %s\n", target_manager_last_error());
      return 7;
    }
    next_id = (unsigned)info[5];
    // what the world says: a target for every object that has appeared and has not been missing for K frames
    long expect = 0, appeared = 0, due = 0;
    for (long i = 0; i < n; ++i) {
      if (first[(size_t)i] <= f && f < last[(size_t)i] + K - 1) ++expect;
      if (first[(size_t)i] == f) ++appeared;
      if (last[(size_t)i] + K - 1 == f) ++due;
    }
    std::printf("frame %ld: %ld detections, %ld born (ids %ld..%ld), %ld retired, %ld targets\n", f, M, info[1], info[4], info[5] - 1, info[0],
                target_manager_size(m));
    if (info[1] != appeared || info[0] != due || target_manager_size(m) != expect) {
      std::printf("  expected %ld born, %ld retired, %ld targets\n", appeared, due, expect);
      ok = false;
    }
  }
  (void)hipFree(det_dev); (void)hipFree(meas_dev); (void)hipFree(has_dev); (void)hipFree(slot_of_det_dev); (void)hipFree(info_dev);
  target_manager_delete(m);
  (void)hipStreamDestroy(stream);
  if (!ok) { std::printf("the population is off\n"); return 8; }
  std::printf("track lifecycle example ok\n");
  return 0;
}
