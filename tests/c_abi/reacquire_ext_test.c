/* reacquire_ext_test.c -- a plain C caller (gcc, C99, no HIP headers) of the re-acquisition calls in
 * include/target_estimation_amd/target_batch_c.h: target_batch_step_sequence_reacquire,
 * target_manager_step_sequence_all_reacquire, target_batch_rejection_runs, target_manager_get_rejection_run.
 * The arithmetic is not re-derived here (tests/test_gpu_reacquire.py holds it to the erase-and-init emulation and to the twin);
 * this program checks the C calling convention: the struct layout, argument order, return values, and that the event rows and
 * the rejection runs follow the contract's table from the NIS rows of the same call.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: reacquire_ext_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipMemset(void* p, int value, size_t bytes);
extern int hipDeviceSynchronize(void);

#define N 300
#define LD 320
#define TICKS 9
#define JUMPED 10
#define GAMMA 300.0
#define K 3

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
  if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ids[N];
  static double p0[N * 7];
  for (int i = 0; i < N; ++i) { ids[i] = 50u + 2u * (unsigned)i; p0[i * 7] = 0.01 * i; p0[i * 7 + 6] = 1.0; }
  if (target_manager_init_batch(m, ids, N, dt, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "init_batch\n"); return 4; }
  target_batch_c* b = target_manager_get_batch(m, 0);
  if (!b || target_batch_size(b) != N) { fprintf(stderr, "batch shape\n"); return 4; }

  /* measurements [TICKS][7][LD]: every target stands still; from tick 3 on the first JUMPED targets are seen 50 m away */
  static double meas[TICKS][7][LD];
  memset(meas, 0, sizeof meas);
  for (int s = 0; s < TICKS; ++s)
    for (int i = 0; i < N; ++i) { meas[s][0][i] = p0[i * 7] + ((s >= 3 && i < JUMPED) ? 50.0 : 0.0); meas[s][6][i] = 1.0; }
  void *meas_dev = NULL, *nis_dev = NULL, *ev_dev = NULL;
  if (hipMalloc(&meas_dev, sizeof meas) || hipMalloc(&nis_dev, sizeof(double) * TICKS * LD) || hipMalloc(&ev_dev, (size_t)TICKS * LD)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(meas_dev, meas, sizeof meas, 1);
  hipMemset(ev_dev, 0xEE, (size_t)TICKS * LD);

  target_innov_stream_c innov = {(double*)nis_dev, NULL, LD, LD, 0, 0};
  target_reacquire_c policy = {K, (unsigned char*)ev_dev, LD, LD, 0};
  /* refusals first: nothing is launched, the message names the cause */
  target_reacquire_c bad = policy;
  bad.max_rejects = 128;
  if (target_batch_step_sequence_reacquire(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov, GAMMA, &bad, 0) >= 0) { fprintf(stderr, "K = 128 accepted\n"); fail = 1; }
  if (target_batch_step_sequence_reacquire(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov, 0.0, &policy, 0) >= 0 ||
      !strstr(target_manager_last_error(), "re-acquisition")) { fprintf(stderr, "a policy without a gate accepted\n"); fail = 1; }
  bad = policy; bad.ld = N - 1;
  if (target_batch_step_sequence_reacquire(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov, GAMMA, &bad, 0) >= 0) { fprintf(stderr, "ld < size accepted\n"); fail = 1; }

  /* ticks 0 .. TICKS-2 through the batch call, the last one through the manager call */
  int rc = target_batch_step_sequence_reacquire(b, TICKS - 1, dt, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov, GAMMA, &policy, 0);
  if (rc != 0) { fprintf(stderr, "target_batch_step_sequence_reacquire: %s\n", target_manager_last_error()); fail = 1; }
  target_batch_sequence_c seq;
  memset(&seq, 0, sizeof seq);
  seq.meas_dev = (char*)meas_dev + sizeof(double) * (size_t)(TICKS - 1) * 7 * LD; seq.tick_stride = 7 * LD; seq.ld = LD;
  target_innov_stream_c innov_last = {(double*)nis_dev + (size_t)(TICKS - 1) * LD, NULL, LD, 0, 0, 0};
  target_reacquire_c policy_last = {K, (unsigned char*)ev_dev + (size_t)(TICKS - 1) * LD, LD, 0, 0};
  const double gate = GAMMA;
  rc = target_manager_step_sequence_all_reacquire(m, 1, dt, &seq, NULL, &innov_last, &gate, &policy_last, 1, 0, NULL, 0.0, 0);
  if (rc != 0) { fprintf(stderr, "target_manager_step_sequence_all_reacquire: %s\n", target_manager_last_error()); fail = 1; }
  hipDeviceSynchronize();

  static double nis[TICKS][LD];
  static unsigned char ev[TICKS][LD], runs[N];
  hipMemcpy(nis, nis_dev, sizeof nis, 2);
  hipMemcpy(ev, ev_dev, sizeof ev, 2);
  if (target_batch_rejection_runs(b, runs) != 0) { fprintf(stderr, "target_batch_rejection_runs: %s\n", target_manager_last_error()); fail = 1; }
  int inits = 0;
  for (int i = 0; i < N && !fail; ++i) {
    unsigned c = 0;
    for (int s = 0; s < TICKS; ++s) {
      unsigned want = 0;
      if (nis[s][i] >= 0.0 && nis[s][i] <= GAMMA) c = 0;
      else { c = c + 1 < 127 ? c + 1 : 127; want = c; if (c >= K) { want = 0x80u | c; c = 0; ++inits; } }
      if (ev[s][i] != want) { fprintf(stderr, "tick %d target %d: event 0x%02x, the table says 0x%02x\n", s, i, ev[s][i], want); fail = 1; break; }
    }
    if (runs[i] != c) { fprintf(stderr, "target %d: run %u, the table says %u\n", i, runs[i], c); fail = 1; }
    if (target_manager_get_rejection_run(m, ids[i]) != (int)c) { fprintf(stderr, "get_rejection_run of id %u\n", ids[i]); fail = 1; }
  }
  for (int s = 0; s < TICKS; ++s)
    for (int i = N; i < LD; ++i)
      if (ev[s][i] != 0xEE) { fprintf(stderr, "event column %d >= size written\n", i); fail = 1; s = TICKS; break; }
  if (ev[5][0] != (0x80u | K) || inits < JUMPED) { fprintf(stderr, "the jumped targets were not re-initialised on tick 5 (%d re-initialisations)\n", inits); fail = 1; }
  if (target_manager_get_rejection_run(m, 7u) >= 0) { fprintf(stderr, "an unknown id has a rejection run\n"); fail = 1; }
  if (target_manager_get_n_measurements(m, ids[0]) != TICKS - K) { fprintf(stderr, "n_measurements of a re-initialised target: %d\n", target_manager_get_n_measurements(m, ids[0])); fail = 1; }
  double pose[7];
  if (!target_manager_get_est_pose(m, ids[0], pose) || !(pose[0] > 40.0)) { fprintf(stderr, "the re-initialised target did not follow the jump: x = %g\n", pose[0]); fail = 1; }
  target_manager_delete(m);
  hipFree(meas_dev); hipFree(nis_dev); hipFree(ev_dev);
  printf(fail ? "REACQUIRE EXT TEST FAILED\n" : "reacquire extension test ok\n");
  return fail;
}
