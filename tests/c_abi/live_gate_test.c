/* live_gate_test.c -- a plain C caller (gcc, C99, no HIP headers) of the gate of the resident sessions in
 * include/target_estimation_amd/target_batch_c.h: target_batch_live_set_gate and target_batch_live_gate_served around
 * target_batch_live_start / _post / _wait / _stop.  The arithmetic is not re-derived here (tests/test_gpu_live_gate.py holds the
 * session to the launched calls and to the twin); this program checks the C calling convention -- the struct layout, argument
 * order, return values -- by running one session that sets the gate, starts, posts tick by tick, reads the NIS and event rows
 * MID-SESSION on a stream of its own, and stops, against target_batch_step_sequence_reacquire through the same ABI on a second
 * manager: rows, rejection runs and poses must be the same bits.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: live_gate_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipMemcpyAsync(void* dst, const void* src, size_t bytes, int kind, void* stream);
extern int hipMemset(void* p, int value, size_t bytes);
extern int hipDeviceSynchronize(void);
extern int hipStreamCreateWithFlags(void** stream, unsigned flags);   /* 1: non-blocking */
extern int hipStreamSynchronize(void* stream);
extern int hipStreamDestroy(void* stream);

#define N 300
#define LD 320
#define TICKS 9
#define RING 4
#define JUMPED 10
#define GAMMA 300.0
#define K 3

static target_batch_c* make(target_manager_c** m, const char* file, const unsigned* ids, double* p0) {
  *m = target_manager_new_ex(file, TARGET_DTYPE_F64, 0);
  if (!*m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return NULL; }
  if (target_manager_init_batch(*m, ids, N, 0.004, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "init_batch\n"); return NULL; }
  target_batch_c* b = target_manager_get_batch(*m, 0);
  if (!b || target_batch_size(b) != N) { fprintf(stderr, "batch shape\n"); return NULL; }
  return b;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ids[N];
  static double p0[N * 7];
  for (int i = 0; i < N; ++i) { ids[i] = 50u + 2u * (unsigned)i; p0[i * 7] = 0.01 * i; p0[i * 7 + 6] = 1.0; }
  target_manager_c *ms = NULL, *ml = NULL;
  target_batch_c* bs = make(&ms, argv[1], ids, p0);   /* the session */
  target_batch_c* bl = make(&ml, argv[1], ids, p0);   /* the launched call */
  if (!bs || !bl) return 4;

  /* measurements [TICKS][7][LD]: every target stands still; from tick 3 on the first JUMPED targets are seen 50 m away */
  static double meas[TICKS][7][LD];
  memset(meas, 0, sizeof meas);
  for (int s = 0; s < TICKS; ++s)
    for (int i = 0; i < N; ++i) { meas[s][0][i] = p0[i * 7] + ((s >= 3 && i < JUMPED) ? 50.0 : 0.0); meas[s][6][i] = 1.0; }
  void *meas_dev = NULL, *nis_l = NULL, *ev_l = NULL, *nis_s = NULL, *ev_s = NULL, *cp = NULL;
  if (hipMalloc(&meas_dev, sizeof meas) || hipMalloc(&nis_l, sizeof(double) * TICKS * LD) || hipMalloc(&ev_l, (size_t)TICKS * LD) ||
      hipMalloc(&nis_s, sizeof(double) * RING * LD) || hipMalloc(&ev_s, (size_t)RING * LD) || hipStreamCreateWithFlags(&cp, 1u)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(meas_dev, meas, sizeof meas, 1);
  hipMemset(ev_l, 0xEE, (size_t)TICKS * LD);
  hipMemset(ev_s, 0xEE, (size_t)RING * LD);
  hipMemset(nis_s, 0xFF, sizeof(double) * RING * LD);

  /* the launched call: every tick's rows */
  target_innov_stream_c innov_l = {(double*)nis_l, NULL, LD, LD, 0, 0};
  target_reacquire_c policy_l = {K, (unsigned char*)ev_l, LD, LD, 0};
  if (target_batch_step_sequence_reacquire(bl, TICKS, dt, meas_dev, 7 * LD, LD, NULL, 0, 0, NULL, &innov_l, GAMMA, &policy_l, 0) != 0) {
    fprintf(stderr, "target_batch_step_sequence_reacquire: %s\n", target_manager_last_error()); return 6; }
  hipDeviceSynchronize();
  static double want_nis[TICKS][LD];
  static unsigned char want_ev[TICKS][LD];
  hipMemcpy(want_nis, nis_l, sizeof want_nis, 2);
  hipMemcpy(want_ev, ev_l, sizeof want_ev, 2);

  /* the session's gate: rows in a ring of RING.  Refusals first: a negative code, the message names the cause */
  target_innov_stream_c rows = {(double*)nis_s, NULL, LD, LD, 0, RING};
  target_reacquire_c policy = {K, (unsigned char*)ev_s, LD, LD, RING};
  if (target_batch_live_gate_served(bs) != 1) { fprintf(stderr, "live_gate_served: %d\n", target_batch_live_gate_served(bs)); fail = 1; }
  if (target_batch_live_gate_served(NULL) != -1) { fprintf(stderr, "live_gate_served(NULL)\n"); fail = 1; }
  const long plain = target_batch_live_capacity(bs);
  target_reacquire_c bad = policy;
  bad.max_rejects = 128;
  if (target_batch_live_set_gate(bs, GAMMA, &rows, &bad) >= 0 || !strstr(target_manager_last_error(), "max_rejects")) { fprintf(stderr, "K = 128 accepted\n"); fail = 1; }
  if (target_batch_live_set_gate(bs, 0.0, &rows, &policy) >= 0 || !strstr(target_manager_last_error(), "needs the gate")) { fprintf(stderr, "a policy without a gate accepted\n"); fail = 1; }
  target_innov_stream_c bad_rows = rows;
  bad_rows.innov_dev = (double*)nis_s;
  if (target_batch_live_set_gate(bs, GAMMA, &bad_rows, NULL) >= 0 || !strstr(target_manager_last_error(), "innov_dev")) { fprintf(stderr, "an innovation block accepted\n"); fail = 1; }
  bad_rows = rows; bad_rows.ld = N - 1; bad_rows.nis_tick_stride = N - 1;
  if (target_batch_live_set_gate(bs, GAMMA, &bad_rows, NULL) >= 0) { fprintf(stderr, "ld < size accepted\n"); fail = 1; }
  if (target_batch_live_capacity(bs) != plain) { fprintf(stderr, "a refused gate changed the capacity\n"); fail = 1; }
  if (target_batch_live_set_gate(bs, GAMMA, &rows, &policy) != 0) { fprintf(stderr, "target_batch_live_set_gate: %s\n", target_manager_last_error()); return 7; }
  const long gated = target_batch_live_capacity(bs);
  if (gated < N || gated > plain) { fprintf(stderr, "live_capacity with a gate: %ld (plain %ld)\n", gated, plain); fail = 1; }

  if (target_batch_live_start(bs, dt, meas_dev, 7 * LD, LD, NULL, 0, TICKS, 0, TICKS, 3.0) != 0) { fprintf(stderr, "target_batch_live_start: %s\n", target_manager_last_error()); return 8; }
  static double got_nis[LD];
  static unsigned char got_ev[LD];
  for (int k = 0; k < TICKS && !fail; ++k) {
    if (target_batch_live_post(bs, 1) != 0 || target_batch_live_wait(bs, k + 1, 5.0) != 0) { fprintf(stderr, "tick %d was not served: %s\n", k, target_manager_last_error()); fail = 1; break; }
    /* rows k % RING, copied on another stream while the session is open */
    hipMemcpyAsync(got_nis, (double*)nis_s + (size_t)(k % RING) * LD, sizeof got_nis, 2, cp);
    hipMemcpyAsync(got_ev, (unsigned char*)ev_s + (size_t)(k % RING) * LD, sizeof got_ev, 2, cp);
    hipStreamSynchronize(cp);
    if (target_batch_live_running(bs) != 1) { fprintf(stderr, "the session ended before tick %d was read\n", k); fail = 1; }
    if (memcmp(got_nis, want_nis[k], sizeof(double) * N) != 0) { fprintf(stderr, "tick %d: the NIS row read mid-session differs from the launched call's\n", k); fail = 1; }
    if (memcmp(got_ev, want_ev[k], N) != 0) { fprintf(stderr, "tick %d: the event row read mid-session differs from the launched call's\n", k); fail = 1; }
    for (int i = N; i < LD; ++i)
      if (got_ev[i] != 0xEE) { fprintf(stderr, "event column %d >= size written\n", i); fail = 1; break; }
  }
  if (target_batch_live_stop(bs) != (fail ? target_batch_live_done(bs) : TICKS) && !fail) { fprintf(stderr, "target_batch_live_stop: %s\n", target_manager_last_error()); fail = 1; }
  if (want_ev[5][0] != (0x80u | K)) { fprintf(stderr, "the jumped targets were not re-initialised on tick 5\n"); fail = 1; }

  static unsigned char runs_s[N], runs_l[N];
  if (target_batch_rejection_runs(bs, runs_s) != 0 || target_batch_rejection_runs(bl, runs_l) != 0) { fprintf(stderr, "target_batch_rejection_runs: %s\n", target_manager_last_error()); fail = 1; }
  if (memcmp(runs_s, runs_l, N) != 0) { fprintf(stderr, "the rejection runs after the session differ from the launched call's\n"); fail = 1; }
  for (int i = 0; i < N && !fail; i += 7) {
    double a[7], c[7];
    if (!target_manager_get_est_pose(ms, ids[i], a) || !target_manager_get_est_pose(ml, ids[i], c) || memcmp(a, c, sizeof a) != 0) { fprintf(stderr, "pose of id %u differs\n", ids[i]); fail = 1; }
    if (target_manager_get_n_measurements(ms, ids[i]) != target_manager_get_n_measurements(ml, ids[i])) { fprintf(stderr, "n_measurements of id %u differs\n", ids[i]); fail = 1; }
    if (target_manager_get_rejection_run(ms, ids[i]) != (int)runs_l[i]) { fprintf(stderr, "get_rejection_run of id %u\n", ids[i]); fail = 1; }
  }
  double pose[7];
  if (!target_manager_get_est_pose(ms, ids[0], pose) || !(pose[0] > 40.0)) { fprintf(stderr, "the re-initialised target did not follow the jump: x = %g\n", pose[0]); fail = 1; }
  /* off again: the capacity is the plain one */
  if (target_batch_live_set_gate(bs, 0.0, NULL, NULL) != 0 || target_batch_live_capacity(bs) != plain) { fprintf(stderr, "switching the gate off\n"); fail = 1; }
  target_manager_delete(ms);
  target_manager_delete(ml);
  hipStreamDestroy(cp);
  hipFree(meas_dev); hipFree(nis_l); hipFree(ev_l); hipFree(nis_s); hipFree(ev_s);
  printf(fail ? "LIVE GATE TEST FAILED\n" : "live gate test ok\n");
  return fail;
}
