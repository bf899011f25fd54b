/* select_soonest_test.c -- a plain C caller (gcc, C99, no HIP headers) of the k-soonest selection in
 * include/target_estimation_amd/target_batch_c.h: target_batch_select_soonest_dev, target_batch_select_soonest and
 * target_manager_select_soonest, behind ticks of target_manager_step_sequence_all with the query on a two-model manager.
 * The program checks the calling convention (argument order, return values, a refusal) and PRINTS what it read back -- every
 * entry of the query's outputs and every row of the three results, doubles as hexadecimal floats -- for
 * tests/test_gpu_select_soonest_c_abi.py to hold against NumPy.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: select_soonest_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipDeviceSynchronize(void);

#define NA 300   /* uniform_acceleration targets (the model file's) */
#define NV 70    /* uniform_velocity targets (typed, diagonal Q / R / P0): they never cross */
#define LD 320
#define TICKS 5
#define KB 5     /* rows of the batch calls */
#define KM 16    /* rows of the manager call */

static double meas[TICKS][7][LD];

static void print_row(const char* form, int i, unsigned id, int batch, int slot, double delta, const double* pose) {
  printf("ROW %s %d %u %d %d %a", form, i, id, batch, slot, delta);
  for (int c = 0; c < 7; ++c) printf(" %a", pose[c]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ida[NA], idv[NV];
  static double pa[NA * 7], pv[NV * 7], va[NA * 6], aa[NA * 6];
  for (int i = 0; i < NA; ++i) { ida[i] = 50u + 2u * (unsigned)i; pa[i * 7] = 8.0 + 0.004 * i; pa[i * 7 + 6] = 1.0; va[i * 6] = -(20.0 + 0.05 * i); aa[i * 6] = 10.0; }
  for (int i = 0; i < NV; ++i) { idv[i] = 5001u + (unsigned)i; pv[i * 7] = 0.01 * i; pv[i * 7 + 6] = 1.0; }
  double Q[36], R[9], P0[36];
  memset(Q, 0, sizeof Q); memset(R, 0, sizeof R); memset(P0, 0, sizeof P0);
  for (int i = 0; i < 6; ++i) { Q[i * 7] = 1e-4; P0[i * 7] = 1.0; }
  for (int i = 0; i < 3; ++i) R[i * 4] = 1e-3;
  /* The query reports the leftmost real root and only if it is not negative: a crossing needs a target outside the sphere (radius 5
   * about the origin) that closes in while it decelerates.  Every target is created with that motion along x -- faster the larger its
   * index, so the crossings differ -- and measured on it. */
  memset(meas, 0, sizeof meas);
  for (int s = 0; s < TICKS; ++s)
    for (int i = 0; i < LD; ++i) {
      const double t = dt * (s + 1);
      meas[s][0][i] = 8.0 + 0.004 * i - (20.0 + 0.05 * i) * t + 5.0 * t * t; meas[s][6][i] = 1.0;
    }
  target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
  if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
  if (target_manager_init_batch(m, ida, NA, dt, 0.0, pa, va, aa) != NA) { fprintf(stderr, "init_batch\n"); return 4; }
  if (target_manager_init_batch_typed(m, TARGET_UNIFORM_VELOCITY, idv, NV, dt, 0.0, Q, R, P0, 0, pv, NULL, NULL) != NV) { fprintf(stderr, "init_batch_typed\n"); return 4; }
  if (target_manager_num_batches(m) != 2) { fprintf(stderr, "expected two batches\n"); return 4; }
  const int n[2] = {NA, NV};
  void *meas_dev = NULL, *delta_dev[2], *pose_dev[2], *ok_dev = NULL;
  if (hipMalloc(&meas_dev, sizeof meas) || hipMalloc(&ok_dev, NA)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(meas_dev, meas, sizeof meas, 1);
  target_batch_sequence_c seq[2];
  memset(seq, 0, sizeof seq);
  for (int b = 0; b < 2; ++b) {
    if (hipMalloc(&delta_dev[b], sizeof(double) * LD) || hipMalloc(&pose_dev[b], sizeof(double) * LD * 7)) { fprintf(stderr, "hipMalloc\n"); return 5; }
    seq[b].meas_dev = meas_dev; seq[b].tick_stride = 7 * LD; seq[b].ld = LD;
    seq[b].delta_dev = (double*)delta_dev[b]; seq[b].pose_dev = (double*)pose_dev[b];
  }
  static unsigned char ok[NA];
  for (int i = 0; i < NA; ++i) ok[i] = (unsigned char)(i % 3 != 0);
  hipMemcpy(ok_dev, ok, NA, 1);
  const double origin[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < TICKS; ++s) {   /* the interceptor's loop: one tick with the query, then the selection behind it */
    seq[0].meas_dev = seq[1].meas_dev = (const char*)meas_dev + sizeof(double) * 7 * LD * (size_t)s;
    if (target_manager_step_sequence_all(m, 1, dt, seq, 2, 1, origin, 5.0, 0) != 0) { fprintf(stderr, "step_sequence_all: %s\n", target_manager_last_error()); return 6; }
  }
  /* what the query left */
  static double delta[2][LD], pose[2][LD * 7];
  static unsigned slot_ids[2][LD];
  hipDeviceSynchronize();
  for (int b = 0; b < 2; ++b) {
    hipMemcpy(delta[b], delta_dev[b], sizeof(double) * (size_t)n[b], 2);
    hipMemcpy(pose[b], pose_dev[b], sizeof(double) * 7 * (size_t)n[b], 2);
    target_batch_c* bh = target_manager_get_batch(m, b);
    if (target_batch_slot_ids(bh, slot_ids[b], LD) != n[b]) { fprintf(stderr, "slot_ids\n"); return 7; }
    printf("N %d %d\n", b, n[b]);
    for (int i = 0; i < n[b]; ++i) {
      printf("E %d %d %u %a", b, i, slot_ids[b][i], delta[b][i]);
      for (int c = 0; c < 7; ++c) printf(" %a", pose[b][i * 7 + c]);
      printf("\n");
    }
  }
  target_batch_c* b0 = target_manager_get_batch(m, 0);
  /* 1. the device form of the batch call, masked, read back by hand */
  {
    void *slot_o = NULL, *delta_o = NULL, *pose_o = NULL, *count_o = NULL;
    if (hipMalloc(&slot_o, sizeof(int) * KB) || hipMalloc(&delta_o, sizeof(double) * KB) || hipMalloc(&pose_o, sizeof(double) * KB * 7) ||
        hipMalloc(&count_o, sizeof(int))) { fprintf(stderr, "hipMalloc\n"); return 5; }
    if (target_batch_select_soonest_dev(b0, (const double*)delta_dev[0], (const double*)pose_dev[0], (const unsigned char*)ok_dev, 0.0, INFINITY, KB,
                                        (int*)slot_o, (double*)delta_o, (double*)pose_o, (int*)count_o) != 0) {
      fprintf(stderr, "select_soonest_dev: %s\n", target_manager_last_error()); return 8;
    }
    hipDeviceSynchronize();
    int slots[KB], count = -5; double d[KB], p[KB * 7];
    hipMemcpy(slots, slot_o, sizeof slots, 2); hipMemcpy(d, delta_o, sizeof d, 2); hipMemcpy(p, pose_o, sizeof p, 2); hipMemcpy(&count, count_o, sizeof count, 2);
    printf("COUNT batch_dev %d\n", count);
    for (int i = 0; i < KB; ++i) print_row("batch_dev", i, slots[i] >= 0 ? slot_ids[0][slots[i]] : 0xffffffffu, slots[i] >= 0 ? 0 : -1, slots[i], d[i], p + i * 7);
    hipFree(slot_o); hipFree(delta_o); hipFree(pose_o); hipFree(count_o);
  }
  /* 2. the host form of the batch call, same inputs: ids filled by the library */
  {
    unsigned ids[KB]; int slots[KB]; double d[KB], p[KB * 7];
    const long count = target_batch_select_soonest(b0, (const double*)delta_dev[0], (const double*)pose_dev[0], (const unsigned char*)ok_dev, 0.0, INFINITY, KB,
                                                   ids, slots, d, p);
    if (count < 0) { fprintf(stderr, "select_soonest: %s\n", target_manager_last_error()); return 8; }
    printf("COUNT batch %ld\n", count);
    for (int i = 0; i < KB; ++i) print_row("batch", i, ids[i], slots[i] >= 0 ? 0 : -1, slots[i], d[i], p + i * 7);
  }
  /* 3. the manager call over both batches, unmasked, without the gather */
  {
    unsigned ids[KM]; int batch[KM], slots[KM]; double d[KM];
    const double none[7] = {0, 0, 0, 0, 0, 0, 1};
    const long count = target_manager_select_soonest(m, seq, 2, NULL, 0.0, INFINITY, KM, ids, batch, slots, d, NULL);
    if (count < 0) { fprintf(stderr, "manager select_soonest: %s\n", target_manager_last_error()); return 8; }
    printf("COUNT manager %ld\n", count);
    for (int i = 0; i < KM; ++i) print_row("manager", i, ids[i], batch[i], slots[i], d[i], none);
  }
  /* a refusal: -1, a message, the arrays untouched */
  {
    unsigned ids[2] = {7u, 7u}; int slots[2] = {-7, -7}; double d[2] = {-7.0, -7.0};
    if (target_batch_select_soonest(b0, (const double*)delta_dev[0], NULL, NULL, -1.0, 1.0, 2, ids, slots, d, NULL) != -1) { printf("a negative delta_lo was not refused\n"); fail = 1; }
    if (!strstr(target_manager_last_error(), "delta_lo")) { printf("the refusal's message: %s\n", target_manager_last_error()); fail = 1; }
    if (ids[0] != 7u || slots[1] != -7 || d[0] != -7.0) { printf("a refused call wrote its outputs\n"); fail = 1; }
    if (target_manager_select_soonest(m, seq, 1, NULL, 0.0, 1.0, 2, ids, slots, slots, d, NULL) != -1) { printf("a wrong number of batches was not refused\n"); fail = 1; }
  }
  target_manager_delete(m);
  hipFree(meas_dev); hipFree(ok_dev);
  for (int b = 0; b < 2; ++b) { hipFree(delta_dev[b]); hipFree(pose_dev[b]); }
  if (fail) return 1;
  printf("select soonest test ok\n");
  return 0;
}
