// soonest_crossings.cpp -- the interceptor's loop of BASELINE configs[4] from plain C++ (no Python, no torch): one GPU's share of the
// population (angular_rates + uniform_acceleration in ONE manager), every tick ONE launch that steps every target and runs its
// own-time sphere query, the convergence gate on the query's device-resident results, and behind it the selection of the k soonest
// converged crossings -- three small launches that leave k rows on the device -- read back once at the end and printed.
// What it replaces in the reference: IntersectionSolver::getIntersectionPoseWithSphere per target (src/intersection_solver.cpp:84-124)
// followed by the caller's own search for the targets to act on.
//   hipcc --offload-arch=gfx950 -O2 -I include/target_estimation_amd examples/soonest_crossings.cpp -o soonest_crossings \
//         -L target_estimation_amd/lib -ltarget_estimation_amd -Wl,-rpath,$PWD/target_estimation_amd/lib
//   ./soonest_crossings models 62500 64 8        (targets per model, ticks, k)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "target_batch_c.h"
#include "target_manager_c.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// Q, R, P0 of a shipped model file, through a throw-away manager that loads it (the reference's YAML format)
static bool model_matrices(const std::string& file, int* type, std::vector<double>& Q, std::vector<double>& R, std::vector<double>& P0) {
  target_manager_c* t = target_manager_new(file.c_str());
  if (!t) return false;
  double one[7] = {0, 0, 0, 0, 0, 0, 1};
  target_manager_init(t, 1u, 0.004, one, 0.0);
  const long n = target_manager_get_n(t, 1u), m = target_manager_get_m(t, 1u);
  *type = target_batch_type(target_manager_get_batch(t, 0));
  Q.assign((size_t)(n * n), 0.0); R.assign((size_t)(m * m), 0.0); P0.assign((size_t)(n * n), 0.0);
  const bool ok = n > 0 && target_manager_get_model_matrices(t, 1u, Q.data(), R.data(), P0.data());
  target_manager_delete(t);
  return ok;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "models";
  const long n = argc > 2 ? std::atol(argv[2]) : 62500;       // targets per model
  const long steps = argc > 3 ? std::atol(argv[3]) : 64;
  const long k = argc > 4 ? std::atol(argv[4]) : 8;
  if (k < 1 || k > TARGET_SOONEST_MAX_K || n < 1 || steps < 1) { std::fprintf(stderr, "usage: %s models n ticks k (1 <= k <= %d)\n", argv[0], TARGET_SOONEST_MAX_K); return 1; }
  const int ticks = 16;                                        // ring of measurements kept in HBM
  const double dt = 0.004, radius = 5.0, origin[3] = {0, 0, 0};   // the generator starts targets in [-10, 10]^3: some of those outside head for the sphere
  const char* files[2] = {"model_angular_rates_params.yaml", "model_uniform_acceleration_params.yaml"};

  target_manager_c* m = target_manager_new_ex(nullptr, TARGET_DTYPE_F32, 0);   // configs[4] is fp32; the query's outputs are doubles either way
  if (!m) return 3;
  hipStream_t stream;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  target_manager_set_stream(m, stream);
  target_batch_sequence_c per_batch[2];
  std::memset(per_batch, 0, sizeof per_batch);
  unsigned char* converged[2] = {nullptr, nullptr};
  std::vector<void*> to_free;
  for (int b = 0; b < 2; ++b) {
    int type = 0;
    std::vector<double> Q, R, P0;
    if (!model_matrices(dir + "/" + files[b], &type, Q, R, P0)) return 4;
    target_stream_c spec;
    std::memset(&spec, 0, sizeof spec);
    spec.model = type; spec.seed = 20240023ull + 17ull * (unsigned)b; spec.first_target = 0; spec.dt = dt; spec.availability = 1.0;
    double* pose0_dev = nullptr;
    HIP_OK(hipMalloc((void**)&pose0_dev, sizeof(double) * 7 * n));
    if (target_stream_truth_dev(&spec, n, pose0_dev, nullptr, nullptr) != 0) return 5;
    std::vector<double> p0((size_t)n * 7);
    HIP_OK(hipMemcpy(p0.data(), pose0_dev, sizeof(double) * 7 * n, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(pose0_dev));
    std::vector<unsigned> ids((size_t)n);
    for (long i = 0; i < n; ++i) ids[(size_t)i] = (unsigned)(i + b * n);
    if (target_manager_init_batch_typed(m, type, ids.data(), n, dt, 0.0, Q.data(), R.data(), P0.data(), 0, p0.data(), nullptr, nullptr) != n) return 6;
    float* meas = nullptr;                                     // SoA [ticks][7][n] in the batch precision
    double *delta = nullptr, *pose = nullptr;
    HIP_OK(hipMalloc((void**)&meas, sizeof(float) * 7 * n * ticks));
    HIP_OK(hipMalloc((void**)&delta, sizeof(double) * n));
    HIP_OK(hipMalloc((void**)&pose, sizeof(double) * 7 * n));
    HIP_OK(hipMalloc((void**)&converged[b], (size_t)n));
    to_free.push_back(meas); to_free.push_back(delta); to_free.push_back(pose); to_free.push_back(converged[b]);
    if (target_stream_fill_dev(&spec, n, 0, ticks, TARGET_DTYPE_F32, meas, 7 * n, n, nullptr, 0, stream) != 0) return 7;
    per_batch[b].meas_dev = meas; per_batch[b].tick_stride = 7 * n; per_batch[b].ld = n;
    per_batch[b].delta_dev = delta; per_batch[b].pose_dev = pose;
  }
  // the k rows of the result, on the device
  int *batch_out = nullptr, *slot_out = nullptr, *count_out = nullptr;
  double *delta_out = nullptr, *pose_out = nullptr;
  HIP_OK(hipMalloc((void**)&batch_out, sizeof(int) * k)); HIP_OK(hipMalloc((void**)&slot_out, sizeof(int) * k)); HIP_OK(hipMalloc((void**)&count_out, sizeof(int)));
  HIP_OK(hipMalloc((void**)&delta_out, sizeof(double) * k)); HIP_OK(hipMalloc((void**)&pose_out, sizeof(double) * 7 * k));
  HIP_OK(hipStreamSynchronize(stream));
  const int one_launch = target_manager_population_tick(m);
  const float* ring[2] = {(const float*)per_batch[0].meas_dev, (const float*)per_batch[1].meas_dev};
  for (long s = 0; s < steps; ++s) {
    // tick + query: one launch for both models
    for (int b = 0; b < 2; ++b) per_batch[b].meas_dev = ring[b] + (size_t)(s % ticks) * 7 * (size_t)n;
    if (target_manager_step_sequence_all(m, 1, dt, per_batch, 2, 1, origin, radius, 0) != 0) return 8;
    // the reference's convergence gate on the results where they are: converged [n] per batch.  (A gate's first error is measured from
    // its initial pose [0 0 0], i.e. it is the radius: nothing converges before that sample has left the window of 4 ticks.)
    for (int b = 0; b < 2; ++b)
      if (target_batch_gate_update_dev(target_manager_get_batch(m, b), per_batch[b].delta_dev, per_batch[b].pose_dev, 3.0, 3.2, 4, converged[b], nullptr, nullptr) != 0) return 9;
    // the k soonest converged crossings within the next two seconds: nothing leaves the device, nothing waits
    const unsigned char* ok[2] = {converged[0], converged[1]};
    if (target_manager_select_soonest_dev(m, per_batch, 2, ok, 0.0, 2.0, k, batch_out, slot_out, delta_out, pose_out, count_out) != 0) {
      std::fprintf(stderr, "select_soonest: %s\n", target_manager_last_error());
      return 10;
    }
  }
  HIP_OK(hipStreamSynchronize(stream));
  std::vector<int> hb((size_t)k), hs((size_t)k);
  std::vector<double> hd((size_t)k), hp((size_t)k * 7);
  int count = 0;
  HIP_OK(hipMemcpy(hb.data(), batch_out, sizeof(int) * k, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hs.data(), slot_out, sizeof(int) * k, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hd.data(), delta_out, sizeof(double) * k, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hp.data(), pose_out, sizeof(double) * 7 * k, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&count, count_out, sizeof(int), hipMemcpyDeviceToHost));
  // slot -> id on the host (valid until the next erase or init of that batch)
  std::vector<unsigned> slot_ids[2];
  for (int b = 0; b < 2; ++b) { slot_ids[b].resize((size_t)n); target_batch_slot_ids(target_manager_get_batch(m, b), slot_ids[b].data(), n); }
  std::printf("%ld + %ld targets (angular_rates + uniform_acceleration, fp32), %ld ticks, %s per tick + gate + selection; after the last tick %d of k = %ld rows:\n",
              n, n, steps, one_launch == 1 ? "ONE launch" : "one launch per batch", count, k);
  bool ordered = true;
  for (long i = 0; i < k; ++i) {
    if (i < count) {
      std::printf("  %2ld  id %7u  batch %d  slot %7d  crosses in %.6f s at [% .4f % .4f % .4f]\n", i, slot_ids[hb[(size_t)i]][(size_t)hs[(size_t)i]], hb[(size_t)i], hs[(size_t)i],
                  hd[(size_t)i], hp[(size_t)i * 7], hp[(size_t)i * 7 + 1], hp[(size_t)i * 7 + 2]);
      if (i > 0 && hd[(size_t)i] < hd[(size_t)i - 1]) ordered = false;
      if (!(hd[(size_t)i] >= 0.0 && hd[(size_t)i] <= 2.0)) ordered = false;
    } else if (hs[(size_t)i] != -1 || hb[(size_t)i] != -1 || hd[(size_t)i] != -1.0 || hp[(size_t)i * 7 + 6] != 1.0) {
      ordered = false;
    }
  }
  for (void* p : to_free) (void)hipFree(p);
  (void)hipFree(batch_out); (void)hipFree(slot_out); (void)hipFree(count_out); (void)hipFree(delta_out); (void)hipFree(pose_out);
  target_manager_delete(m);
  (void)hipStreamDestroy(stream);
  if (!ordered) { std::printf("the rows are not in order\n"); return 11; }
  std::printf("soonest crossings example ok\n");
  return 0;
}
