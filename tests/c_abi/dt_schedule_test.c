/* dt_schedule_test.c -- a plain C caller (gcc, C99, no HIP headers) of the calls with a time step per tick in
 * include/target_estimation_amd/target_batch_c.h: target_batch_step_sequence_dt, target_batch_step_fused_dt,
 * target_batch_step_fused_dt_served and target_manager_step_sequence_all_dt.
 * The arithmetic is not re-derived here (tests/test_gpu_dt_schedule.py holds it to the single ticks and to the twin); this program
 * checks the C calling convention: argument order, the structs, return values, and that each of the three stepping calls leaves
 * the same bytes -- state, covariance, measurement counter, time, pose -- as TICKS calls of target_batch_step with dt_host[s] on
 * another manager; and with the gate, the same NIS rows, event rows and rejection runs as the gated single ticks.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: dt_schedule_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
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
#define NS 9     /* state dimension of uniform_acceleration */
#define HOWS 4   /* 0: single ticks; 1: step_sequence_dt; 2: step_fused_dt; 3: step_sequence_all_dt */

static double x[HOWS][N * NS], P[HOWS][N * NS * NS], tm[HOWS][N], pose[HOWS][7];
static int nm[HOWS][N];
static double nis[3][TICKS][LD];
static unsigned char ev[3][TICKS][LD], runs[3][N];

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt0 = 0.004;
  /* jitter, a tick at exactly 0.0, a late frame of 3 dt */
  const double sched[TICKS] = {0.004, 0.0031, 0.0, 0.0052, 0.012, 0.001, 0.0078, 0.004, 0.0044};
  static unsigned ids[N];
  static double p0[N * 7];
  for (int i = 0; i < N; ++i) { ids[i] = 50u + 2u * (unsigned)i; p0[i * 7] = 0.01 * i; p0[i * 7 + 6] = 1.0; }
  /* measurements [TICKS][7][LD]: every target drifts slowly; from tick 3 on the first JUMPED targets are seen 50 m away */
  static double meas[TICKS][7][LD];
  memset(meas, 0, sizeof meas);
  for (int s = 0; s < TICKS; ++s)
    for (int i = 0; i < N; ++i) { meas[s][0][i] = p0[i * 7] + 0.001 * s + ((s >= 3 && i < JUMPED) ? 50.0 : 0.0); meas[s][6][i] = 1.0; }
  void *meas_dev = NULL, *nis_dev = NULL, *ev_dev = NULL;
  if (hipMalloc(&meas_dev, sizeof meas) || hipMalloc(&nis_dev, sizeof nis[0]) || hipMalloc(&ev_dev, sizeof ev[0])) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(meas_dev, meas, sizeof meas, 1);
  const char* const what[HOWS] = {"single ticks", "step_sequence_dt", "step_fused_dt", "step_sequence_all_dt"};
  /* ---- the plain calls against target_batch_step */
  for (int how = 0; how < HOWS; ++how) {
    target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
    if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
    if (target_manager_init_batch(m, ids, N, dt0, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "init_batch\n"); return 4; }
    target_batch_c* b = target_manager_get_batch(m, 0);
    if (!b || target_batch_size(b) != N) { fprintf(stderr, "batch shape\n"); return 4; }
    int rc = 0;
    if (how == 0) {
      for (int s = 0; s < TICKS && rc == 0; ++s) rc = target_batch_step(b, sched[s], (const char*)meas_dev + (size_t)s * 7 * LD * sizeof(double), LD, NULL);
    } else if (how == 1) {
      if (target_batch_step_sequence_dt(b, TICKS, NULL, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, NULL, 0.0, NULL, 0) >= 0 ||
          !strstr(target_manager_last_error(), "dt_host")) { fprintf(stderr, "step_sequence_dt: a NULL schedule accepted\n"); fail = 1; }
      if (target_batch_step_sequence_dt(b, TICKS, sched, meas_dev, 7 * LD, LD, NULL, 0, -1, NULL, NULL, 0.0, NULL, 0) >= 0) { fprintf(stderr, "a negative ring accepted\n"); fail = 1; }
      rc = target_batch_step_sequence_dt(b, TICKS, sched, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, NULL, 0.0, NULL, 0);
    } else if (how == 2) {
      if (target_batch_step_fused_dt(b, TICKS, NULL, meas_dev, 7 * LD, LD, NULL, 0, NULL, NULL, 0.0, NULL) >= 0 ||
          !strstr(target_manager_last_error(), "dt_host")) { fprintf(stderr, "step_fused_dt: a NULL schedule accepted\n"); fail = 1; }
      if (target_batch_step_fused_dt(b, TICKS, sched, meas_dev, 7 * LD, N - 1, NULL, 0, NULL, NULL, 0.0, NULL) >= 0) { fprintf(stderr, "ld < size accepted\n"); fail = 1; }
      /* two calls back to back, no synchronisation between them: each reads its own part of the schedule */
      rc = target_batch_step_fused_dt(b, 4, sched, meas_dev, 7 * LD, LD, NULL, 0, NULL, NULL, 0.0, NULL);
      if (rc == 0) rc = target_batch_step_fused_dt(b, TICKS - 4, sched + 4, (const char*)meas_dev + (size_t)4 * 7 * LD * sizeof(double), 7 * LD, LD, NULL, 0, NULL, NULL, 0.0, NULL);
      /* (asked after the first fused call: a batch in the shared-axes form says 0 until that call has expanded it) */
      if (target_batch_step_fused_dt_served(b, 0) != 1 || target_batch_step_fused_dt_served(b, 1) != 1) { fprintf(stderr, "the automatic fp64 layout is not served by one launch\n"); fail = 1; }
    } else {
      target_batch_sequence_c spec = {meas_dev, 7 * LD, LD, NULL, 0, NULL, NULL, 0};
      if (target_manager_step_sequence_all_dt(m, TICKS, NULL, &spec, NULL, NULL, NULL, NULL, 1, 0, NULL, 0.0, 0) >= 0 ||
          !strstr(target_manager_last_error(), "dt_host")) { fprintf(stderr, "step_sequence_all_dt: a NULL schedule accepted\n"); fail = 1; }
      rc = target_manager_step_sequence_all_dt(m, TICKS, sched, &spec, NULL, NULL, NULL, NULL, 1, 0, NULL, 0.0, 1);
    }
    if (rc != 0) { fprintf(stderr, "%s: %s\n", what[how], target_manager_last_error()); fail = 1; }
    if (target_manager_get_state_batch(m, ids, N, x[how], P[how]) != NS) { fprintf(stderr, "get_state_batch\n"); fail = 1; }
    for (int i = 0; i < N; ++i) {
      nm[how][i] = target_manager_get_n_measurements(m, ids[i]);
      if (target_manager_get_time(m, ids[i], &tm[how][i]) != 0) { fprintf(stderr, "get_time\n"); fail = 1; break; }
    }
    if (!target_manager_get_est_pose(m, ids[N - 1], pose[how])) { fprintf(stderr, "get_est_pose\n"); fail = 1; }
    target_manager_delete(m);
  }
  for (int how = 1; how < HOWS; ++how) {
    if (memcmp(x[how], x[0], sizeof x[0])) { fprintf(stderr, "%s: the state differs from the single ticks'\n", what[how]); fail = 1; }
    if (memcmp(P[how], P[0], sizeof P[0])) { fprintf(stderr, "%s: the covariance differs from the single ticks'\n", what[how]); fail = 1; }
    if (memcmp(nm[how], nm[0], sizeof nm[0])) { fprintf(stderr, "%s: the measurement counters differ from the single ticks'\n", what[how]); fail = 1; }
    if (memcmp(tm[how], tm[0], sizeof tm[0])) { fprintf(stderr, "%s: the times differ from the single ticks' (%.17g, %.17g)\n", what[how], tm[how][0], tm[0][0]); fail = 1; }
    if (memcmp(pose[how], pose[0], sizeof pose[0])) { fprintf(stderr, "%s: the estimated pose differs from the single ticks'\n", what[how]); fail = 1; }
  }
  double sum = 0.0;
  for (int s = 0; s < TICKS; ++s) sum += sched[s];
  if (!(tm[0][0] > sum - 1e-12 && tm[0][0] < sum + 1e-12) || nm[0][0] != TICKS) { fprintf(stderr, "time %.17g (the schedule sums to %.17g), %d measurements\n", tm[0][0], sum, nm[0][0]); fail = 1; }
  /* ---- the gated calls against the gated single ticks: NIS rows, event rows, runs */
  for (int how = 0; how < 3; ++how) {
    target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
    if (!m || target_manager_init_batch(m, ids, N, dt0, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "manager\n"); return 4; }
    target_batch_c* b = target_manager_get_batch(m, 0);
    hipMemset(nis_dev, 0xEE, sizeof nis[0]); hipMemset(ev_dev, 0xEE, sizeof ev[0]);
    target_innov_stream_c innov = {(double*)nis_dev, NULL, LD, LD, 0, 0};
    target_reacquire_c policy = {K, (unsigned char*)ev_dev, LD, LD, 0};
    int rc = 0;
    if (how == 0) {
      for (int s = 0; s < TICKS && rc == 0; ++s) {
        target_innov_stream_c row = {(double*)nis_dev + (size_t)s * LD, NULL, LD, LD, 0, 0};
        target_reacquire_c pol = {K, (unsigned char*)ev_dev + (size_t)s * LD, LD, LD, 0};
        rc = target_batch_step_sequence_reacquire(b, 1, sched[s], (const char*)meas_dev + (size_t)s * 7 * LD * sizeof(double), 7 * LD, LD, NULL, 0, 0, NULL,
                                                  &row, GAMMA, &pol, 0);
      }
    } else if (how == 1) {
      rc = target_batch_step_sequence_dt(b, TICKS, sched, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov, GAMMA, &policy, 1);
    } else {
      if (target_batch_step_fused_dt(b, TICKS, sched, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov, 0.0, &policy) >= 0) { fprintf(stderr, "a policy without a gate accepted\n"); fail = 1; }
      rc = target_batch_step_fused_dt(b, TICKS, sched, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov, GAMMA, &policy);
    }
    if (rc != 0) { fprintf(stderr, "gated %s: %s\n", what[how], target_manager_last_error()); fail = 1; }
    hipDeviceSynchronize();
    hipMemcpy(nis[how], nis_dev, sizeof nis[0], 2);
    hipMemcpy(ev[how], ev_dev, sizeof ev[0], 2);
    if (target_batch_rejection_runs(b, runs[how]) != 0) { fprintf(stderr, "target_batch_rejection_runs: %s\n", target_manager_last_error()); fail = 1; }
    target_manager_delete(m);
  }
  for (int how = 1; how < 3; ++how) {
    if (memcmp(nis[how], nis[0], sizeof nis[0])) { fprintf(stderr, "gated %s: the NIS rows differ from the single ticks'\n", what[how]); fail = 1; }
    if (memcmp(ev[how], ev[0], sizeof ev[0])) { fprintf(stderr, "gated %s: the event rows differ from the single ticks'\n", what[how]); fail = 1; }
    if (memcmp(runs[how], runs[0], sizeof runs[0])) { fprintf(stderr, "gated %s: the rejection runs differ from the single ticks'\n", what[how]); fail = 1; }
  }
  if (ev[2][5][0] != (0x80u | K)) { fprintf(stderr, "the jumped targets were not re-initialised on tick 5: event 0x%02x\n", ev[2][5][0]); fail = 1; }
  for (int i = N; i < LD; ++i)
    if (ev[2][TICKS - 1][i] != 0xEE) { fprintf(stderr, "event column %d >= size written\n", i); fail = 1; break; }
  if (target_batch_step_fused_dt_served(NULL, 0) != -1) { fprintf(stderr, "a NULL handle is served\n"); fail = 1; }
  hipFree(meas_dev); hipFree(nis_dev); hipFree(ev_dev);
  printf(fail ? "DT SCHEDULE TEST FAILED\n" : "dt schedule test ok\n");
  return fail;
}
