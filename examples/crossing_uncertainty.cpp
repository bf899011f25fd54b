// crossing_uncertainty.cpp -- "which targets cross the sphere soonest, and how well is that known", from plain C++ (no Python, no
// torch), everything on the device: one GPU's share of BASELINE configs[4] (angular_rates + uniform_acceleration in ONE manager),
// and per tick
//   1  ONE launch that steps every target and runs its own-time sphere query            (target_manager_step_sequence_all)
//   2  per batch, the position covariance at every crossing, its radial spread sigma_r, the spread sigma_t of the crossing time,
//      and the mask "known to within sigma_t_max"                                        (target_batch_crossing_cov_dev, dense)
//   3  the k soonest crossings among the masked ones                                     (target_manager_select_soonest_dev)
//   4  the covariance and the spreads of those k rows                                    (target_manager_crossing_cov_dev, rows)
// and one read-back of the k rows at the end.  The mask is the filter's own statement about its uncertainty; the reference's
// moving-average convergence gate (examples/soonest_crossings.cpp) only sees how much the answer moved.
//   hipcc --offload-arch=gfx950 -O2 -I include/target_estimation_amd examples/crossing_uncertainty.cpp -o crossing_uncertainty \
//         -L target_estimation_amd/lib -ltarget_estimation_amd -Wl,-rpath,$PWD/target_estimation_amd/lib
//   ./crossing_uncertainty models 62500 64 8 0.002        (targets per model, ticks, k, sigma_t_max in seconds)
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
  const double sigma_t_max = argc > 5 ? std::atof(argv[5]) : 0.002;
  if (k < 1 || k > TARGET_SOONEST_MAX_K || n < 1 || steps < 1 || !(sigma_t_max >= 0.0)) {
    std::fprintf(stderr, "usage: %s models n ticks k sigma_t_max (1 <= k <= %d)\n", argv[0], TARGET_SOONEST_MAX_K);
    return 1;
  }
  const int ticks = 16;                                        // ring of measurements kept in HBM
  const double dt = 0.004, radius = 5.0, origin[3] = {0, 0, 0};   // the generator starts targets in [-10, 10]^3: some of those outside head for the sphere
  const double nan = std::nan(""), inf = INFINITY;
  const char* files[2] = {"model_angular_rates_params.yaml", "model_uniform_acceleration_params.yaml"};

  target_manager_c* m = target_manager_new_ex(nullptr, TARGET_DTYPE_F32, 0);   // configs[4] is fp32; covariance and spreads come out as doubles either way
  if (!m) return 3;
  hipStream_t stream;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  target_manager_set_stream(m, stream);
  target_batch_sequence_c per_batch[2];
  std::memset(per_batch, 0, sizeof per_batch);
  double* cov[2] = {nullptr, nullptr};
  double* sigma[2] = {nullptr, nullptr};
  unsigned char* known[2] = {nullptr, nullptr};
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
    HIP_OK(hipMalloc((void**)&cov[b], sizeof(double) * 6 * n));
    HIP_OK(hipMalloc((void**)&sigma[b], sizeof(double) * 2 * n));
    HIP_OK(hipMalloc((void**)&known[b], (size_t)n));
    to_free.push_back(meas); to_free.push_back(delta); to_free.push_back(pose); to_free.push_back(cov[b]); to_free.push_back(sigma[b]); to_free.push_back(known[b]);
    if (target_stream_fill_dev(&spec, n, 0, ticks, TARGET_DTYPE_F32, meas, 7 * n, n, nullptr, 0, stream) != 0) return 7;
    per_batch[b].meas_dev = meas; per_batch[b].tick_stride = 7 * n; per_batch[b].ld = n;
    per_batch[b].delta_dev = delta; per_batch[b].pose_dev = pose;
  }
  // the k rows of the result, on the device
  int *batch_out = nullptr, *slot_out = nullptr, *count_out = nullptr;
  double *delta_out = nullptr, *pose_out = nullptr, *cov_out = nullptr, *sigma_out = nullptr;
  HIP_OK(hipMalloc((void**)&batch_out, sizeof(int) * k)); HIP_OK(hipMalloc((void**)&slot_out, sizeof(int) * k)); HIP_OK(hipMalloc((void**)&count_out, sizeof(int)));
  HIP_OK(hipMalloc((void**)&delta_out, sizeof(double) * k)); HIP_OK(hipMalloc((void**)&pose_out, sizeof(double) * 7 * k));
  HIP_OK(hipMalloc((void**)&cov_out, sizeof(double) * 6 * k)); HIP_OK(hipMalloc((void**)&sigma_out, sizeof(double) * 2 * k));
  HIP_OK(hipStreamSynchronize(stream));
  const float* ring[2] = {(const float*)per_batch[0].meas_dev, (const float*)per_batch[1].meas_dev};
  for (long s = 0; s < steps; ++s) {
    // 1  tick + query: one launch for both models
    for (int b = 0; b < 2; ++b) per_batch[b].meas_dev = ring[b] + (size_t)(s % ticks) * 7 * (size_t)n;
    if (target_manager_step_sequence_all(m, 1, dt, per_batch, 2, 1, origin, radius, 0) != 0) return 8;
    // 2  what the filter knows about every crossing: known[i] = delta >= 0 && sigma_t <= sigma_t_max.  t1 = NaN: the query was at each
    //    target's own time.  A target that does not cross costs its delta and nothing else.
    for (int b = 0; b < 2; ++b)
      if (target_batch_crossing_cov_dev(target_manager_get_batch(m, b), nan, origin, radius, per_batch[b].delta_dev, nullptr, n, inf, sigma_t_max,
                                        cov[b], sigma[b], known[b]) != 0) {
        std::fprintf(stderr, "crossing_cov: %s\n", target_manager_last_error());
        return 9;
      }
    // 3  the k soonest of those within the next two seconds
    const unsigned char* ok[2] = {known[0], known[1]};
    if (target_manager_select_soonest_dev(m, per_batch, 2, ok, 0.0, 2.0, k, batch_out, slot_out, delta_out, pose_out, count_out) != 0) return 10;
    // 4  their covariance and spreads, k rows (a filler row of the selection gives a filler row here)
    if (target_manager_crossing_cov_dev(m, nan, origin, radius, batch_out, slot_out, delta_out, k, inf, inf, cov_out, sigma_out, nullptr) != 0) {
      std::fprintf(stderr, "crossing_cov (rows): %s\n", target_manager_last_error());
      return 11;
    }
  }
  HIP_OK(hipStreamSynchronize(stream));
  std::vector<int> hb((size_t)k), hs((size_t)k);
  std::vector<double> hd((size_t)k), hp((size_t)k * 7), hc((size_t)k * 6), hg((size_t)k * 2);
  int count = 0;
  HIP_OK(hipMemcpy(hb.data(), batch_out, sizeof(int) * k, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hs.data(), slot_out, sizeof(int) * k, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hd.data(), delta_out, sizeof(double) * k, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hp.data(), pose_out, sizeof(double) * 7 * k, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hc.data(), cov_out, sizeof(double) * 6 * k, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hg.data(), sigma_out, sizeof(double) * 2 * k, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&count, count_out, sizeof(int), hipMemcpyDeviceToHost));
  std::vector<unsigned> slot_ids[2];
  for (int b = 0; b < 2; ++b) { slot_ids[b].resize((size_t)n); target_batch_slot_ids(target_manager_get_batch(m, b), slot_ids[b].data(), n); }
  std::printf("%ld + %ld targets (angular_rates + uniform_acceleration, fp32), %ld ticks; after the last tick %d of k = %ld crossings known to within %g s:\n",
              n, n, steps, count, k, sigma_t_max);
  bool good = true;
  for (long i = 0; i < k; ++i) {
    const size_t u = (size_t)i;
    if (i < count) {
      std::printf("  %2ld  id %7u  crosses in %.6f s +- %.3f ms at [% .4f % .4f % .4f] +- %.2f mm along the normal\n", i, slot_ids[hb[u]][(size_t)hs[u]], hd[u],
                  1e3 * hg[u * 2 + 1], hp[u * 7], hp[u * 7 + 1], hp[u * 7 + 2], 1e3 * hg[u * 2]);
      if (i > 0 && hd[u] < hd[u - 1]) good = false;
      if (!(hg[u * 2 + 1] <= sigma_t_max) || !(hg[u * 2] >= 0.0)) good = false;      // the mask let only such rows through
    } else if (hs[u] != -1 || hg[u * 2] != -1.0 || hg[u * 2 + 1] != -1.0 || hc[u * 6] != 0.0) {
      good = false;
    }
    // the same row for a program to read: doubles as hexadecimal floats
    std::printf("ROW %ld %u %d %d %a", i, i < count ? slot_ids[hb[u]][(size_t)hs[u]] : ~0u, hb[u], hs[u], hd[u]);
    for (int c = 0; c < 6; ++c) std::printf(" %a", hc[u * 6 + (size_t)c]);
    std::printf(" %a %a\n", hg[u * 2], hg[u * 2 + 1]);
  }
  for (void* p : to_free) (void)hipFree(p);
  (void)hipFree(batch_out); (void)hipFree(slot_out); (void)hipFree(count_out); (void)hipFree(delta_out); (void)hipFree(pose_out);
  (void)hipFree(cov_out); (void)hipFree(sigma_out);
  target_manager_delete(m);
  (void)hipStreamDestroy(stream);
  if (!good) { std::printf("the rows are not what the mask and the order promise\n"); return 12; }
  std::printf("crossing uncertainty example ok\n");
  return 0;
}
