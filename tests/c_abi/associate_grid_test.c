/* associate_grid_test.c -- a plain C caller (gcc, C99, no HIP headers) of the grid form of the association in
 * include/target_estimation_amd/target_batch_c.h: target_batch_associate_grid_dev, target_batch_associate_grid,
 * target_manager_associate_grid_dev and target_manager_associate_grid, on a two-model manager, followed by the tick that consumes
 * the scattered measurements.  The program checks the calling convention itself: every detection sits on one target's predicted
 * position (reversed order, so that a wrong pairing shows), some are clutter, so the pairing is known; the brute-force sibling on
 * the same frame must give the same per-detection rows; info[3] counts the wide slots: none with a huge cell, all with a tiny one.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: associate_grid_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipDeviceSynchronize(void);

#define NA 70    /* uniform_acceleration targets (the model file's), on the line y = 0 */
#define NV 40    /* uniform_velocity targets (typed), on the line y = 5 */
#define CL 7     /* clutter detections, far from everything */
#define MM (NA + NV + CL)
#define LD 96
#define GATE 9.0
#define BIG_CELL 1.0e3    /* every slot narrow, everything near in a few cells */
#define TINY_CELL 1.0e-6  /* every slot wide */

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); fail = 1; } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ida[NA], idv[NV];
  static double pa[NA * 7], pv[NV * 7];
  for (int i = 0; i < NA; ++i) { ida[i] = 50u + 2u * (unsigned)i; pa[i * 7] = 0.5 * i; pa[i * 7 + 6] = 1.0; }
  for (int i = 0; i < NV; ++i) { idv[i] = 5001u + (unsigned)i; pv[i * 7] = 0.5 * i; pv[i * 7 + 1] = 5.0; pv[i * 7 + 6] = 1.0; }
  double Q[36], R[9], P0[36];
  memset(Q, 0, sizeof Q); memset(R, 0, sizeof R); memset(P0, 0, sizeof P0);
  for (int i = 0; i < 6; ++i) { Q[i * 7] = 1e-6; P0[i * 7] = 1e-2; }
  for (int i = 0; i < 3; ++i) R[i * 4] = 2.5e-3;
  if (TARGET_ASSOC_GRID_MAX_DETECTIONS != 1048576) { fprintf(stderr, "TARGET_ASSOC_GRID_MAX_DETECTIONS\n"); return 3; }
  target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
  if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
  if (target_manager_init_batch(m, ida, NA, dt, 0.0, pa, NULL, NULL) != NA) { fprintf(stderr, "init_batch\n"); return 4; }
  if (target_manager_init_batch_typed(m, TARGET_UNIFORM_VELOCITY, idv, NV, dt, 0.0, Q, R, P0, 0, pv, NULL, NULL) != NV) { fprintf(stderr, "init_batch_typed\n"); return 4; }
  if (target_manager_num_batches(m) != 2) { fprintf(stderr, "expected two batches\n"); return 4; }
  const int n[2] = {NA, NV};
  static double det[MM * 7];
  static int want_batch[MM], want_slot[MM];
  for (int j = 0; j < MM; ++j) {
    double* d = det + j * 7;
    d[6] = 1.0;
    if (j < NA) { want_batch[j] = 0; want_slot[j] = NA - 1 - j; d[0] = 0.5 * (NA - 1 - j) + 0.01; d[1] = 0.0; }
    else if (j < NA + NV) { want_batch[j] = 1; want_slot[j] = NA + NV - 1 - j; d[0] = 0.5 * (NA + NV - 1 - j); d[1] = 5.0 - 0.01; }
    else { want_batch[j] = -1; want_slot[j] = -1; d[0] = 3.0 * j; d[1] = 100.0; d[2] = -50.0; }
  }
  void *det_dev = NULL, *meas_dev[2], *has_dev[2], *dos_dev[2], *d2s_dev[2], *sod_dev = NULL, *bod_dev = NULL, *d2d_dev = NULL, *info_dev = NULL;
  if (hipMalloc(&det_dev, sizeof det) || hipMalloc(&sod_dev, sizeof(int) * MM) || hipMalloc(&bod_dev, sizeof(int) * MM) ||
      hipMalloc(&d2d_dev, sizeof(double) * MM) || hipMalloc(&info_dev, sizeof(int) * 4)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  for (int b = 0; b < 2; ++b)
    if (hipMalloc(&meas_dev[b], sizeof(double) * 7 * LD) || hipMalloc(&has_dev[b], LD) || hipMalloc(&dos_dev[b], sizeof(int) * LD) ||
        hipMalloc(&d2s_dev[b], sizeof(double) * LD)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(det_dev, det, sizeof det, 1);
  target_batch_c* bh[2] = {target_manager_get_batch(m, 0), target_manager_get_batch(m, 1)};
  static int sod[MM], bod[MM], info[4], dos[LD], sod_brute[MM], bod_brute[MM];
  static double d2d[MM], d2s[LD], meas[7 * LD], d2d_brute[MM];
  static unsigned char has[LD];
  target_assoc_out_c per[2];
  for (int b = 0; b < 2; ++b) {
    per[b].meas_out_dev = meas_dev[b]; per[b].ld = LD; per[b].has_meas_out_dev = (unsigned char*)has_dev[b];
    per[b].det_of_slot_dev = (int*)dos_dev[b]; per[b].d2_of_slot_dev = (double*)d2s_dev[b];
  }

  /* 0. the brute-force sibling on the same frame: what the grid form must reproduce */
  if (target_manager_associate_dev(m, dt, (const double*)det_dev, MM, GATE, 4, per, 2, (int*)sod_dev, (int*)bod_dev, (double*)d2d_dev,
                                   (int*)info_dev) != 0) { fprintf(stderr, "manager associate_dev: %s\n", target_manager_last_error()); return 6; }
  hipDeviceSynchronize();
  hipMemcpy(sod_brute, sod_dev, sizeof sod, 2); hipMemcpy(bod_brute, bod_dev, sizeof bod, 2); hipMemcpy(d2d_brute, d2d_dev, sizeof d2d, 2);

  /* 1. the manager's device form with both extremes of cell, then the tick that consumes its output */
  const double cells[2] = {TINY_CELL, BIG_CELL};
  for (int k = 0; k < 2; ++k) {
    if (target_manager_associate_grid_dev(m, dt, (const double*)det_dev, MM, GATE, 4, cells[k], per, 2, (int*)sod_dev, (int*)bod_dev,
                                          (double*)d2d_dev, (int*)info_dev) != 0) { fprintf(stderr, "manager associate_grid_dev: %s\n", target_manager_last_error()); return 6; }
    hipDeviceSynchronize();
    hipMemcpy(sod, sod_dev, sizeof sod, 2); hipMemcpy(bod, bod_dev, sizeof bod, 2); hipMemcpy(d2d, d2d_dev, sizeof d2d, 2);
    hipMemcpy(info, info_dev, sizeof info, 2);
    if (info[0] != NA + NV || info[1] < 1 || info[2] != 1 || info[3] != (k == 0 ? NA + NV : 0)) FAIL("manager_dev cell %g info %d %d %d %d", cells[k], info[0], info[1], info[2], info[3]);
    if (memcmp(sod, sod_brute, sizeof sod) || memcmp(bod, bod_brute, sizeof bod) || memcmp(d2d, d2d_brute, sizeof d2d)) FAIL("manager_dev cell %g differs from the brute-force form", cells[k]);
    for (int j = 0; j < MM; ++j) {
      if (sod[j] != want_slot[j] || bod[j] != want_batch[j]) FAIL("manager_dev det %d -> batch %d slot %d, want %d %d", j, bod[j], sod[j], want_batch[j], want_slot[j]);
      if (want_slot[j] >= 0 ? !(d2d[j] >= 0.0 && d2d[j] <= GATE) : d2d[j] != -1.0) FAIL("manager_dev d2 of det %d: %g", j, d2d[j]);
    }
  }
  for (int b = 0; b < 2; ++b) {
    hipMemcpy(dos, dos_dev[b], sizeof(int) * (size_t)n[b], 2); hipMemcpy(d2s, d2s_dev[b], sizeof(double) * (size_t)n[b], 2);
    hipMemcpy(has, has_dev[b], (size_t)n[b], 2); hipMemcpy(meas, meas_dev[b], sizeof meas, 2);
    for (int i = 0; i < n[b]; ++i) {
      const int j = dos[i];
      if (j < 0 || want_batch[j] != b || want_slot[j] != i || has[i] != 1) { FAIL("manager_dev batch %d slot %d -> det %d", b, i, j); continue; }
      if (memcmp(&d2s[i], &d2d[j], sizeof(double)) != 0) FAIL("the two d2 of pair (%d, %d) differ: %a %a", i, j, d2s[i], d2d[j]);
      for (int c = 0; c < 7; ++c)
        if (meas[c * LD + i] != det[j * 7 + c]) FAIL("batch %d slot %d word %d: %g, want %g", b, i, c, meas[c * LD + i], det[j * 7 + c]);
    }
    if (target_batch_step(bh[b], dt, meas_dev[b], LD, (const unsigned char*)has_dev[b]) != 0) { fprintf(stderr, "step: %s\n", target_manager_last_error()); return 7; }
  }
  /* 2. the batch's device form: batch 1 alone sees the whole frame and takes its own 40 detections.  Its S is 0.0125 per axis
   * (P0 + Q + R) and a little more after the tick: reach below 0.4, so every slot is narrow at cell 0.5 */
  {
    if (target_batch_associate_grid_dev(bh[1], dt, (const double*)det_dev, MM, GATE, 4, 0.5, meas_dev[1], LD, (unsigned char*)has_dev[1],
                                        (int*)dos_dev[1], NULL, (int*)sod_dev, NULL, (int*)info_dev) != 0) { fprintf(stderr, "batch associate_grid_dev: %s\n", target_manager_last_error()); return 6; }
    hipDeviceSynchronize();
    hipMemcpy(sod, sod_dev, sizeof sod, 2); hipMemcpy(info, info_dev, sizeof info, 2);
    if (info[0] != NV || info[2] != 1 || info[3] != 0) FAIL("batch_dev info %d %d %d %d", info[0], info[1], info[2], info[3]);
    for (int j = 0; j < MM; ++j)
      if (sod[j] != (want_batch[j] == 1 ? want_slot[j] : -1)) FAIL("batch_dev det %d -> slot %d", j, sod[j]);
  }
  /* 3. the host forms: ids, the unmatched list, the return value */
  {
    static unsigned ids[MM]; static long unmatched[MM]; long nu = -1;
    const long got = target_batch_associate_grid(bh[0], dt, det, MM, GATE, 4, BIG_CELL, NULL, 0, NULL, ids, sod, d2d, unmatched, &nu, info);
    if (got != NA || nu != NV + CL || info[0] != NA || info[3] != 0) FAIL("batch host form: %ld matched, %ld unmatched (%s)", got, nu, target_manager_last_error());
    for (int j = 0; j < MM; ++j)
      if (ids[j] != (want_batch[j] == 0 ? ida[want_slot[j]] : 0xffffffffu)) FAIL("batch host form det %d -> id %u", j, ids[j]);
    for (long k = 0; k < nu; ++k)
      if (unmatched[k] != NA + k) FAIL("batch host form unmatched[%ld] = %ld", k, unmatched[k]);
    nu = -1;
    const long gm = target_manager_associate_grid(m, dt, det, MM, GATE, 4, TINY_CELL, NULL, 0, ids, bod, sod, d2d, unmatched, &nu, info);
    if (gm != NA + NV || nu != CL || info[2] != 1 || info[3] != NA + NV) FAIL("manager host form: %ld matched, %ld unmatched (%s)", gm, nu, target_manager_last_error());
    for (int j = 0; j < MM; ++j) {
      const unsigned want = want_batch[j] == 0 ? ida[want_slot[j]] : want_batch[j] == 1 ? idv[want_slot[j]] : 0xffffffffu;
      if (ids[j] != want || bod[j] != want_batch[j] || sod[j] != want_slot[j]) FAIL("manager host form det %d -> id %u batch %d slot %d", j, ids[j], bod[j], sod[j]);
    }
    for (long k = 0; k < nu; ++k)
      if (unmatched[k] != NA + NV + k) FAIL("manager host form unmatched[%ld] = %ld", k, unmatched[k]);
    /* M == 0 is no error; the wide count is still reported */
    if (target_manager_associate_grid(m, dt, NULL, 0, GATE, 4, BIG_CELL, NULL, 0, NULL, NULL, NULL, NULL, NULL, &nu, info) != 0 || nu != 0 ||
        info[0] != 0 || info[1] != 0 || info[2] != 1 || info[3] != 0) FAIL("M == 0: %s", target_manager_last_error());
  }
  /* refusals: -1, a message, nothing written */
  {
    int keep[4] = {-7, -7, -7, -7};
    hipMemcpy(info_dev, keep, sizeof keep, 1);
    if (target_batch_associate_grid_dev(bh[0], dt, (const double*)det_dev, MM, GATE, 4, 0.5, meas_dev[0], NA - 1, (unsigned char*)has_dev[0], NULL, NULL,
                                        NULL, NULL, (int*)info_dev) != -1 || !strstr(target_manager_last_error(), "ld")) FAIL("ld < size was not refused: %s", target_manager_last_error());
    if (target_batch_associate_grid_dev(bh[0], dt, (const double*)det_dev, MM, HUGE_VAL, 4, 0.5, meas_dev[0], LD, (unsigned char*)has_dev[0], NULL, NULL,
                                        NULL, NULL, (int*)info_dev) != -1 || !strstr(target_manager_last_error(), "gate")) FAIL("an infinite gate was not refused");
    if (target_batch_associate_grid_dev(bh[0], dt, (const double*)det_dev, MM, GATE, 4, 0.0, meas_dev[0], LD, (unsigned char*)has_dev[0], NULL, NULL,
                                        NULL, NULL, (int*)info_dev) != -1 || !strstr(target_manager_last_error(), "cell")) FAIL("cell 0 was not refused");
    if (target_manager_associate_grid_dev(m, dt, (const double*)det_dev, MM, GATE, 4, 0.5, NULL, 1, NULL, NULL, NULL, (int*)info_dev) != -1) FAIL("a wrong number of batches was not refused");
    hipDeviceSynchronize();
    hipMemcpy(info, info_dev, sizeof info, 2);
    if (info[0] != -7 || info[2] != -7 || info[3] != -7) FAIL("a refused call wrote info");
  }
  target_manager_delete(m);
  hipFree(det_dev); hipFree(sod_dev); hipFree(bod_dev); hipFree(d2d_dev); hipFree(info_dev);
  for (int b = 0; b < 2; ++b) { hipFree(meas_dev[b]); hipFree(has_dev[b]); hipFree(dos_dev[b]); hipFree(d2s_dev[b]); }
  if (fail) return 1;
  printf("associate grid test ok\n");
  return 0;
}
