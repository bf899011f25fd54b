/* fused_gate_test.c -- a plain C caller (gcc, C99, no HIP headers) of the gate inside a temporally fused call in
 * include/target_estimation_amd/target_batch_c.h: target_batch_step_fused_gated and target_batch_step_fused_gate_served.
 * The arithmetic is not re-derived here (tests/test_gpu_fused_gate.py holds it to the single ticks and to the twin); this
 * program checks the C calling convention: argument order, the structs, return values, and that one fused call leaves the same
 * bytes -- NIS rows, innovation blocks, event rows, rejection runs, poses -- as target_batch_step_sequence_reacquire called with
 * the same arguments on a second manager.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: fused_gate_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
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
#define M 3

static double nis[2][TICKS][LD], nu[2][TICKS][M][LD];
static unsigned char ev[2][TICKS][LD], runs[2][N];

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ids[N];
  static double p0[N * 7];
  for (int i = 0; i < N; ++i) { ids[i] = 50u + 2u * (unsigned)i; p0[i * 7] = 0.01 * i; p0[i * 7 + 6] = 1.0; }
  /* measurements [TICKS][7][LD]: every target stands still; from tick 3 on the first JUMPED targets are seen 50 m away */
  static double meas[TICKS][7][LD];
  memset(meas, 0, sizeof meas);
  for (int s = 0; s < TICKS; ++s)
    for (int i = 0; i < N; ++i) { meas[s][0][i] = p0[i * 7] + ((s >= 3 && i < JUMPED) ? 50.0 : 0.0); meas[s][6][i] = 1.0; }
  void *meas_dev = NULL, *nis_dev = NULL, *nu_dev = NULL, *ev_dev = NULL;
  if (hipMalloc(&meas_dev, sizeof meas) || hipMalloc(&nis_dev, sizeof nis[0]) || hipMalloc(&nu_dev, sizeof nu[0]) || hipMalloc(&ev_dev, sizeof ev[0])) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(meas_dev, meas, sizeof meas, 1);
  target_manager_c* mgr[2] = {NULL, NULL};
  double pose[2][7];
  for (int how = 0; how < 2; ++how) {   /* 0: one fused call; 1: the sequence */
    target_manager_c* m = mgr[how] = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
    if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
    if (target_manager_init_batch(m, ids, N, dt, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "init_batch\n"); return 4; }
    target_batch_c* b = target_manager_get_batch(m, 0);
    if (!b || target_batch_size(b) != N) { fprintf(stderr, "batch shape\n"); return 4; }
    hipMemset(nis_dev, 0xEE, sizeof nis[0]); hipMemset(nu_dev, 0xEE, sizeof nu[0]); hipMemset(ev_dev, 0xEE, sizeof ev[0]);
    target_innov_stream_c innov = {(double*)nis_dev, (double*)nu_dev, LD, LD, M * LD, 0};
    target_reacquire_c policy = {K, (unsigned char*)ev_dev, LD, LD, 0};
    int rc;
    if (how == 0) {
      if (target_batch_step_fused_gate_served(b) != 1) { fprintf(stderr, "the automatic fp64 layout is not served by one launch\n"); fail = 1; }
      /* refusals first: nothing is launched, the message names the cause */
      target_reacquire_c bad = policy;
      bad.max_rejects = 128;
      if (target_batch_step_fused_gated(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov, GAMMA, &bad) >= 0) { fprintf(stderr, "K = 128 accepted\n"); fail = 1; }
      if (target_batch_step_fused_gated(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov, 0.0, &policy) >= 0 ||
          !strstr(target_manager_last_error(), "re-acquisition")) { fprintf(stderr, "a policy without a gate accepted\n"); fail = 1; }
      if (target_batch_step_fused_gated(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, NULL, NULL, GAMMA, NULL) >= 0) { fprintf(stderr, "a gate without a stream accepted\n"); fail = 1; }
      if (target_batch_step_fused_gated(b, 1L << 31, dt, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov, GAMMA, &policy) >= 0) { fprintf(stderr, "n_ticks beyond an int accepted\n"); fail = 1; }
      hipMemcpy(ev[0], ev_dev, sizeof ev[0], 2);
      if (ev[0][0][0] != 0xEE || ev[0][TICKS - 1][N - 1] != 0xEE) { fprintf(stderr, "a refused call wrote event rows\n"); fail = 1; }
      rc = target_batch_step_fused_gated(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov, GAMMA, &policy);
    } else {
      rc = target_batch_step_sequence_reacquire(b, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov, GAMMA, &policy, 0);
    }
    if (rc != 0) { fprintf(stderr, "call %d: %s\n", how, target_manager_last_error()); fail = 1; }
    hipDeviceSynchronize();
    hipMemcpy(nis[how], nis_dev, sizeof nis[0], 2);
    hipMemcpy(nu[how], nu_dev, sizeof nu[0], 2);
    hipMemcpy(ev[how], ev_dev, sizeof ev[0], 2);
    if (target_batch_rejection_runs(b, runs[how]) != 0) { fprintf(stderr, "target_batch_rejection_runs: %s\n", target_manager_last_error()); fail = 1; }
    if (!target_manager_get_est_pose(m, ids[0], pose[how])) { fprintf(stderr, "get_est_pose\n"); fail = 1; }
  }
  if (memcmp(nis[0], nis[1], sizeof nis[0])) { fprintf(stderr, "the NIS rows differ from the sequence's\n"); fail = 1; }
  if (memcmp(nu[0], nu[1], sizeof nu[0])) { fprintf(stderr, "the innovation blocks differ from the sequence's\n"); fail = 1; }
  if (memcmp(ev[0], ev[1], sizeof ev[0])) { fprintf(stderr, "the event rows differ from the sequence's\n"); fail = 1; }
  if (memcmp(runs[0], runs[1], sizeof runs[0])) { fprintf(stderr, "the rejection runs differ from the sequence's\n"); fail = 1; }
  if (memcmp(pose[0], pose[1], sizeof pose[0])) { fprintf(stderr, "the estimated pose differs from the sequence's\n"); fail = 1; }
  int inits = 0;
  for (int i = 0; i < N && !fail; ++i) {   /* the contract's table from the fused call's own NIS rows */
    unsigned c = 0;
    for (int s = 0; s < TICKS; ++s) {
      unsigned want = 0;
      if (nis[0][s][i] >= 0.0 && nis[0][s][i] <= GAMMA) c = 0;
      else { c = c + 1 < 127 ? c + 1 : 127; want = c; if (c >= K) { want = 0x80u | c; c = 0; ++inits; } }
      if (ev[0][s][i] != want) { fprintf(stderr, "tick %d target %d: event 0x%02x, the table says 0x%02x\n", s, i, ev[0][s][i], want); fail = 1; break; }
    }
    if (runs[0][i] != c) { fprintf(stderr, "target %d: run %u, the table says %u\n", i, runs[0][i], c); fail = 1; }
    if (target_manager_get_rejection_run(mgr[0], ids[i]) != (int)c) { fprintf(stderr, "get_rejection_run of id %u\n", ids[i]); fail = 1; }
  }
  for (int s = 0; s < TICKS; ++s)
    for (int i = N; i < LD; ++i)
      if (ev[0][s][i] != 0xEE) { fprintf(stderr, "event column %d >= size written\n", i); fail = 1; s = TICKS; break; }
  if (ev[0][5][0] != (0x80u | K) || inits < JUMPED) { fprintf(stderr, "the jumped targets were not re-initialised on tick 5 (%d re-initialisations)\n", inits); fail = 1; }
  if (target_manager_get_n_measurements(mgr[0], ids[0]) != TICKS - K) { fprintf(stderr, "n_measurements of a re-initialised target: %d\n", target_manager_get_n_measurements(mgr[0], ids[0])); fail = 1; }
  if (!(pose[0][0] > 40.0)) { fprintf(stderr, "the re-initialised target did not follow the jump: x = %g\n", pose[0][0]); fail = 1; }
  if (target_batch_step_fused_gate_served(NULL) != -1) { fprintf(stderr, "a NULL handle is served\n"); fail = 1; }
  target_manager_delete(mgr[0]); target_manager_delete(mgr[1]);
  hipFree(meas_dev); hipFree(nis_dev); hipFree(nu_dev); hipFree(ev_dev);
  printf(fail ? "FUSED GATE TEST FAILED\n" : "fused gate test ok\n");
  return fail;
}
