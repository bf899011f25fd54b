/* fused_all_test.c -- a plain C caller (gcc, C99, no HIP headers) of the manager-level fused replay in
 * include/target_estimation_amd/target_batch_c.h: target_manager_step_fused_all, ..._all_dt and ..._all_served.
 * The arithmetic is not re-derived here (tests/test_gpu_fused_all.py holds it to the per-batch calls and to the oracle); this
 * program checks the C calling convention: argument order, the per-batch arrays, return values, and that one manager-level call on
 * a two-model manager leaves the same bytes -- NIS rows, event rows, rejection runs, poses, times -- as target_batch_step_fused_gated
 * / target_batch_step_fused_dt called batch by batch with the same arguments on a second manager.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: fused_all_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipMemset(void* p, int value, size_t bytes);
extern int hipDeviceSynchronize(void);

#define NA 300   /* uniform_acceleration targets (the model file's) */
#define NV 70    /* uniform_velocity targets (typed, diagonal Q / R / P0) */
#define LD 320
#define TICKS 9
#define JUMPED 10
#define GAMMA 300.0
#define K 3

static double nis[2][2][TICKS][LD];         /* [how][batch] */
static unsigned char ev[2][2][TICKS][LD], runs[2][2][NA];
static double meas[TICKS][7][LD];

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  const double dts[TICKS] = {0.004, 0.003, 0.0052, 0.0, 0.004, 0.01, 0.004, 0.0037, 0.004};
  static unsigned ida[NA], idv[NV];
  static double pa[NA * 7], pv[NV * 7];
  for (int i = 0; i < NA; ++i) { ida[i] = 50u + 2u * (unsigned)i; pa[i * 7] = 0.01 * i; pa[i * 7 + 6] = 1.0; }
  for (int i = 0; i < NV; ++i) { idv[i] = 5001u + (unsigned)i; pv[i * 7] = 0.01 * i; pv[i * 7 + 6] = 1.0; }
  double Q[36], R[9], P0[36];
  memset(Q, 0, sizeof Q); memset(R, 0, sizeof R); memset(P0, 0, sizeof P0);
  for (int i = 0; i < 6; ++i) { Q[i * 7] = 1e-4; P0[i * 7] = 1.0; }
  for (int i = 0; i < 3; ++i) R[i * 4] = 1e-3;
  /* measurements [TICKS][7][LD], shared by both batches: every target stands still; from tick 3 on the first JUMPED targets are seen 50 m away */
  memset(meas, 0, sizeof meas);
  for (int s = 0; s < TICKS; ++s)
    for (int i = 0; i < NA; ++i) { meas[s][0][i] = 0.01 * i + ((s >= 3 && i < JUMPED) ? 50.0 : 0.0); meas[s][6][i] = 1.0; }
  void *meas_dev = NULL, *nis_dev[2] = {NULL, NULL}, *ev_dev[2] = {NULL, NULL};
  if (hipMalloc(&meas_dev, sizeof meas)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  for (int b = 0; b < 2; ++b)
    if (hipMalloc(&nis_dev[b], sizeof nis[0][0]) || hipMalloc(&ev_dev[b], sizeof ev[0][0])) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(meas_dev, meas, sizeof meas, 1);
  target_manager_c* mgr[2] = {NULL, NULL};
  double pose[2][2][7], tim[2][2];
  for (int how = 0; how < 2; ++how) {   /* 0: the manager-level calls; 1: batch by batch */
    target_manager_c* m = mgr[how] = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
    if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
    if (target_manager_init_batch(m, ida, NA, dt, 0.0, pa, NULL, NULL) != NA) { fprintf(stderr, "init_batch\n"); return 4; }
    if (target_manager_init_batch_typed(m, 3, idv, NV, dt, 0.0, Q, R, P0, 0, pv, NULL, NULL) != NV) { fprintf(stderr, "init_batch_typed: %s\n", target_manager_last_error()); return 4; }
    if (target_manager_num_batches(m) != 2) { fprintf(stderr, "two batches expected\n"); return 4; }
    target_batch_c* bt[2] = {target_manager_get_batch(m, 0), target_manager_get_batch(m, 1)};
    if (target_batch_size(bt[0]) != NA || target_batch_size(bt[1]) != NV) { fprintf(stderr, "batch shape\n"); return 4; }
    for (int b = 0; b < 2; ++b) { hipMemset(nis_dev[b], 0xEE, sizeof nis[0][0]); hipMemset(ev_dev[b], 0xEE, sizeof ev[0][0]); }
    target_batch_sequence_c seq[2];
    memset(seq, 0, sizeof seq);
    target_innov_stream_c innov[2];
    target_reacquire_c policy[2];
    const double gates[2] = {GAMMA, GAMMA};
    for (int b = 0; b < 2; ++b) {
      seq[b].meas_dev = meas_dev; seq[b].tick_stride = 7 * LD; seq[b].ld = LD;
      target_innov_stream_c in = {(double*)nis_dev[b], NULL, LD, LD, 0, 0};
      target_reacquire_c po = {b == 0 ? K : -1, b == 0 ? (unsigned char*)ev_dev[b] : NULL, LD, LD, 0};   /* batch 1: no policy */
      innov[b] = in; policy[b] = po;
    }
    int rc = 0;
    if (how == 0) {
      if (target_manager_step_fused_all_served(m, 0, 0) != 1 || target_manager_step_fused_all_served(m, 1, 1) != 1) { fprintf(stderr, "a two-model fp64 manager is not served by one launch\n"); fail = 1; }
      /* refusals first: nothing is launched or changed, the message names the cause */
      seq[1].ring_ticks = 4;
      if (target_manager_step_fused_all(m, TICKS, dt, seq, NULL, innov, gates, policy, 2) >= 0 || !strstr(target_manager_last_error(), "ring_ticks")) { fprintf(stderr, "ring_ticks != 0 accepted\n"); fail = 1; }
      seq[1].ring_ticks = 0;
      if (target_manager_step_fused_all(m, TICKS, dt, seq, NULL, innov, gates, policy, 1) >= 0) { fprintf(stderr, "one spec for two batches accepted\n"); fail = 1; }
      if (target_manager_step_fused_all(m, TICKS, dt, seq, NULL, innov, NULL, policy, 2) >= 0 || !strstr(target_manager_last_error(), "re-acquisition")) { fprintf(stderr, "a policy without a gate accepted\n"); fail = 1; }
      if (target_manager_step_fused_all_dt(m, TICKS, NULL, seq, NULL, innov, gates, policy, 2) >= 0 || !strstr(target_manager_last_error(), "dt_host")) { fprintf(stderr, "dt_host NULL accepted\n"); fail = 1; }
      hipMemcpy(ev[0][0], ev_dev[0], sizeof ev[0][0], 2);
      if (ev[0][0][0][0] != 0xEE || ev[0][0][TICKS - 1][NA - 1] != 0xEE || target_batch_shared_axes(bt[0]) != 1) { fprintf(stderr, "a refused call changed something\n"); fail = 1; }
      rc = target_manager_step_fused_all(m, TICKS, dt, seq, NULL, innov, gates, policy, 2);
      if (rc == 0) rc = target_manager_step_fused_all_dt(m, TICKS, dts, seq, NULL, NULL, NULL, NULL, 2);   /* the plain loop with a schedule */
      if (target_batch_shared_axes(bt[0]) != 0 || target_batch_shared_axes(bt[1]) != 0) { fprintf(stderr, "the call did not expand the shared-axes batches\n"); fail = 1; }
    } else {
      for (int b = 0; b < 2 && rc == 0; ++b)
        rc = target_batch_step_fused_gated(bt[b], TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, NULL, &innov[b], gates[b], b == 0 ? &policy[b] : NULL);
      for (int b = 0; b < 2 && rc == 0; ++b)
        rc = target_batch_step_fused_dt(bt[b], TICKS, dts, meas_dev, 7 * LD, LD, NULL, 0, NULL, NULL, 0.0, NULL);
    }
    if (rc != 0) { fprintf(stderr, "call %d: %s\n", how, target_manager_last_error()); fail = 1; }
    hipDeviceSynchronize();
    for (int b = 0; b < 2; ++b) {
      hipMemcpy(nis[how][b], nis_dev[b], sizeof nis[0][0], 2);
      hipMemcpy(ev[how][b], ev_dev[b], sizeof ev[0][0], 2);
      if (target_batch_rejection_runs(bt[b], runs[how][b]) != 0) { fprintf(stderr, "target_batch_rejection_runs: %s\n", target_manager_last_error()); fail = 1; }
      const unsigned id = b == 0 ? ida[0] : idv[NV - 1];
      if (!target_manager_get_est_pose(m, id, pose[how][b])) { fprintf(stderr, "get_est_pose\n"); fail = 1; }
      if (target_manager_get_time(m, id, &tim[how][b]) < 0) { fprintf(stderr, "get_time\n"); fail = 1; }
    }
  }
  if (memcmp(nis[0], nis[1], sizeof nis[0])) { fprintf(stderr, "the NIS rows differ from the per-batch calls'\n"); fail = 1; }
  if (memcmp(ev[0], ev[1], sizeof ev[0])) { fprintf(stderr, "the event rows differ from the per-batch calls'\n"); fail = 1; }
  if (memcmp(runs[0], runs[1], sizeof runs[0])) { fprintf(stderr, "the rejection runs differ from the per-batch calls'\n"); fail = 1; }
  if (memcmp(pose[0], pose[1], sizeof pose[0])) { fprintf(stderr, "the estimated poses differ from the per-batch calls'\n"); fail = 1; }
  if (memcmp(tim[0], tim[1], sizeof tim[0])) { fprintf(stderr, "the times differ from the per-batch calls'\n"); fail = 1; }
  double want_t = 0.0;
  for (int s = 0; s < TICKS; ++s) want_t += dt + dts[s];
  if (!(tim[0][0] > want_t - 1e-12 && tim[0][0] < want_t + 1e-12)) { fprintf(stderr, "time %.17g, expected %.17g\n", tim[0][0], want_t); fail = 1; }
  if (ev[0][0][5][0] != (0x80u | K)) { fprintf(stderr, "the jumped targets were not re-initialised on tick 5: 0x%02x\n", ev[0][0][5][0]); fail = 1; }
  if (ev[0][1][0][0] != 0xEE) { fprintf(stderr, "a batch without a policy wrote event rows\n"); fail = 1; }
  unsigned char pad[sizeof(double)];
  memset(pad, 0xEE, sizeof pad);
  if (!(nis[0][1][4][0] > GAMMA) || memcmp(&nis[0][1][4][NV], pad, sizeof pad)) { fprintf(stderr, "batch 1: NIS row of tick 4 (columns >= size must stay untouched)\n"); fail = 1; }
  if (target_manager_step_fused_all_served(NULL, 0, 0) != -1) { fprintf(stderr, "a NULL handle is served\n"); fail = 1; }
  if (target_manager_step_fused_all(NULL, 1, dt, NULL, NULL, NULL, NULL, NULL, 0) >= 0) { fprintf(stderr, "a NULL manager accepted\n"); fail = 1; }
  target_manager_delete(mgr[0]); target_manager_delete(mgr[1]);
  hipFree(meas_dev);
  for (int b = 0; b < 2; ++b) { hipFree(nis_dev[b]); hipFree(ev_dev[b]); }
  printf(fail ? "FUSED ALL TEST FAILED\n" : "fused all test ok\n");
  return fail;
}
