// duplicate_tracks.cpp -- track_lifecycle.cpp's tracker with a detector that SPLITS some objects into two detections for a few
// frames.  One of the two matches the object's track, the other is born as a new target (the lifecycle's rule 2), and from then on
// two tracks follow one object: they take turns winning its one detection, so neither reaches max_misses.  Two managers see the
// same frames; one of them also calls target_manager_retire_duplicates behind the lifecycle.  The program prints both populations.
// What it replaces: reading every state and covariance back, a spatial join on the host, and erase_batch.
// (min_hits = 0 here: the lattice is 4 m wide, so a newborn's wide P0 reaches nobody but its twin.  A tracker in dense scenes
// would ask for a hit or two first.)
//   hipcc --offload-arch=gfx950 -O2 -I include/target_estimation_amd examples/duplicate_tracks.cpp -o duplicate_tracks \
//         -L target_estimation_amd/lib -ltarget_estimation_amd -Wl,-rpath,$PWD/target_estimation_amd/lib
//   ./duplicate_tracks models 2000 8        (objects, frames)
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
  if (n < 10 || n > 500000 || frames < 4) { std::fprintf(stderr, "usage: %s models n frames (10 <= n <= 500000, frames >= 4)\n", argv[0]); return 1; }
  const double dt = 0.004, noise = 0.001, gate = 9.0, cell = 2.0, split = 0.01;
  const int rounds = 4, K = 2;
  const long cap = 2 * n;   // the most targets either manager can hold
  target_manager_c* mgr[2];
  hipStream_t stream;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  for (int w = 0; w < 2; ++w) {
    mgr[w] = target_manager_new_ex((dir + "/model_uniform_velocity_params.yaml").c_str(), TARGET_DTYPE_F64, 0);
    if (!mgr[w]) return 3;
    target_manager_set_stream(mgr[w], stream);
  }
  std::mt19937_64 rng(2026);
  std::normal_distribution<double> gauss(0.0, noise);
  double *det_dev = nullptr, *meas_dev = nullptr;
  unsigned char* has_dev = nullptr;
  int *slot_of_det_dev = nullptr, *info_dev = nullptr;
  HIP_OK(hipMalloc((void**)&det_dev, sizeof(double) * 7 * cap)); HIP_OK(hipMalloc((void**)&meas_dev, sizeof(double) * 7 * cap));
  HIP_OK(hipMalloc((void**)&has_dev, (size_t)cap)); HIP_OK(hipMalloc((void**)&slot_of_det_dev, sizeof(int) * cap));
  HIP_OK(hipMalloc((void**)&info_dev, sizeof(int) * 4));
  target_assoc_out_c per;
  std::memset(&per, 0, sizeof per);
  per.meas_out_dev = meas_dev; per.ld = cap; per.has_meas_out_dev = has_dev;
  target_batch_sequence_c seq;
  std::memset(&seq, 0, sizeof seq);
  seq.meas_dev = meas_dev; seq.tick_stride = 7 * cap; seq.ld = cap; seq.has_meas_dev = has_dev; seq.has_stride = cap;
  const unsigned char* masks[1] = {has_dev};
  target_lifecycle_c policy;
  std::memset(&policy, 0, sizeof policy);
  policy.max_misses = K;
  policy.birth_type = TARGET_UNIFORM_VELOCITY;
  policy.max_births = cap;
  policy.dt0 = dt;
  std::vector<unsigned> retired((size_t)cap), kept((size_t)cap);
  std::vector<double> frame;
  unsigned next_id[2] = {1, 1};
  long most_without = 0, retired_total = 0, splits_total = 0;
  bool ok = true;
  for (long f = 0; f < frames; ++f) {
    // the frame: every object once; in frames 1 .. 3 every tenth object twice, `split` apart
    const bool splitting = f >= 1 && f <= 3;
    frame.clear();
    long splits = 0;
    for (long i = 0; i < n; ++i) {
      const double x = 4.0 * (double)(i % 64), y = 4.0 * (double)((i / 64) % 64), z = 4.0 * (double)(i / 4096);
      const int copies = (splitting && i % 10 == 0) ? 2 : 1;
      splits += copies - 1;
      for (int c = 0; c < copies; ++c) {
        const double off = copies == 2 ? (c == 0 ? -0.5 * split : 0.5 * split) : 0.0;
        const double d[7] = {x + off + gauss(rng), y + gauss(rng), z + gauss(rng), 0.0, 0.0, 0.0, 1.0};
        frame.insert(frame.end(), d, d + 7);
      }
    }
    const long M = (long)frame.size() / 7;
    HIP_OK(hipMemcpyAsync(det_dev, frame.data(), sizeof(double) * 7 * M, hipMemcpyHostToDevice, stream));
    long size[2] = {0, 0};
    for (int w = 0; w < 2; ++w) {
      target_manager_c* m = mgr[w];
      const int nb = target_manager_num_batches(m);
      if (target_manager_associate_grid_dev(m, dt, det_dev, M, gate, rounds, cell, &per, nb, slot_of_det_dev, nullptr, nullptr, info_dev) != 0) {
        std::fprintf(stderr, "associate: %s\n", target_manager_last_error());
        return 5;
      }
      if (nb > 0 && target_manager_step_sequence_all(m, 1, dt, &seq, nb, 0, nullptr, 0.0, 0) != 0) {
        std::fprintf(stderr, "step: %s\n", target_manager_last_error());
        return 6;
      }
      policy.first_id = next_id[w];
      policy.t_birth = dt * (double)(f + 1);
      long info[6];
      if (target_manager_lifecycle(m, det_dev, slot_of_det_dev, M, masks, nb, &policy, retired.data(), cap, info) != 0) {
        std::fprintf(stderr, "lifecycle: %s\n", target_manager_last_error());
        return 7;
      }
      next_id[w] = (unsigned)info[5];
      if (w == 0) {
        // ... and the duplicates go, on the device: only the counts and the two id lists come back
        long dinfo[4];
        if (target_manager_retire_duplicates(m, dt, gate, rounds, cell, 0, retired.data(), kept.data(), cap, dinfo) != 0) {
          std::fprintf(stderr, "retire_duplicates: %s\n", target_manager_last_error());
          return 8;
        }
        retired_total += dinfo[0];
        if (dinfo[3] != 0) { std::printf("  %ld wide rows: the cell is too small\n", dinfo[3]); ok = false; }
      }
      size[w] = target_manager_size(m);
    }
    splits_total += splits;
    most_without = std::max(most_without, size[1]);
    std::printf("frame %ld: %ld detections (%ld objects split): %ld targets with retire_duplicates, %ld without\n", f, M, splits, size[0], size[1]);
    if (size[0] != n) { std::printf("  expected %ld targets with the call\n", n); ok = false; }
  }
  std::printf("%ld objects; %ld duplicate tracks retired; without the call the population reached %ld\n", n, retired_total, most_without);
  if (most_without <= n || retired_total < 1 || retired_total > splits_total) ok = false;
  (void)hipFree(det_dev); (void)hipFree(meas_dev); (void)hipFree(has_dev); (void)hipFree(slot_of_det_dev); (void)hipFree(info_dev);
  for (int w = 0; w < 2; ++w) target_manager_delete(mgr[w]);
  (void)hipStreamDestroy(stream);
  if (!ok) { std::printf("the population is off\n"); return 9; }
  std::printf("duplicate tracks example ok\n");
  return 0;
}
