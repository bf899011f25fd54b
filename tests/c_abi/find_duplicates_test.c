/* find_duplicates_test.c -- a plain C caller (gcc, C99, no HIP headers) of the duplicate-track search in
 * include/target_estimation_amd/target_batch_c.h: target_manager_find_duplicates_dev and target_manager_retire_duplicates.
 * The program checks the calling convention itself: N targets 4 m apart with two hits each, then TWINS targets 1 cm next to the
 * first TWINS of them with one hit each, so who is the duplicate of whom, and where the survivors end up, is known.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: find_duplicates_test <uniform_velocity model.yaml>   (exit code 0 = pass) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipMemset(void* p, int value, size_t bytes);
extern int hipDeviceSynchronize(void);

#define N 70
#define TWINS 3
#define ALL (N + TWINS)
#define LD 128
#define GATE 9.0
#define CELL 2.0

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); fail = 1; } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ids[ALL];
  static double p0[ALL * 7];
  for (int i = 0; i < ALL; ++i) {
    ids[i] = i < N ? 100u + (unsigned)i : 9000u + (unsigned)(i - N);
    p0[i * 7] = i < N ? 4.0 * i : 4.0 * (i - N) + 0.01;
    p0[i * 7 + 6] = 1.0;
  }
  target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
  if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
  if (target_manager_init_batch(m, ids, ALL, dt, 0.0, p0, NULL, NULL) != ALL) { fprintf(stderr, "init_batch\n"); return 4; }
  void *has_dev = NULL, *dup_dev = NULL, *pb_dev = NULL, *ps_dev = NULL, *d2_dev = NULL, *info_dev = NULL;
  if (hipMalloc(&has_dev, LD) || hipMalloc(&dup_dev, LD) || hipMalloc(&pb_dev, sizeof(int) * LD) || hipMalloc(&ps_dev, sizeof(int) * LD) ||
      hipMalloc(&d2_dev, sizeof(double) * LD) || hipMalloc(&info_dev, sizeof(int) * 4)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  /* counters through the lifecycle's retirement half: everybody is seen once, the first N a second time */
  static unsigned char mask[LD];
  const unsigned char* masks[1] = {(const unsigned char*)has_dev};
  target_lifecycle_c pol;
  memset(&pol, 0, sizeof pol);
  pol.birth_type = -1;
  long linfo[6];
  for (int call = 0; call < 2; ++call) {
    for (int i = 0; i < ALL; ++i) mask[i] = (unsigned char)(call == 0 || i < N);
    hipMemcpy(has_dev, mask, LD, 1);
    if (target_manager_lifecycle(m, NULL, NULL, 0, masks, 1, &pol, NULL, 0, linfo) != 0) { fprintf(stderr, "lifecycle: %s\n", target_manager_last_error()); return 6; }
  }
  target_dup_out_c per;
  memset(&per, 0, sizeof per);
  per.dup_out_dev = (unsigned char*)dup_dev; per.partner_batch_dev = (int*)pb_dev; per.partner_slot_dev = (int*)ps_dev; per.d2_of_slot_dev = (double*)d2_dev;
  static unsigned char dup[LD];
  static int pb[LD], ps[LD], info[4];
  static double d2[LD];
  /* min_hits 2: the twins are not eligible, nothing pairs */
  if (target_manager_find_duplicates_dev(m, dt, GATE, 4, CELL, 2, &per, 1, (int*)info_dev) != 0) { fprintf(stderr, "find: %s\n", target_manager_last_error()); return 7; }
  hipDeviceSynchronize();
  hipMemcpy(info, info_dev, sizeof info, 2);
  if (info[0] != 0 || info[1] != 1 || info[2] != 1 || info[3] != 0) FAIL("min_hits 2: info %d %d %d %d", info[0], info[1], info[2], info[3]);
  /* min_hits 1: TWINS pairs; the twin has fewer hits and is the duplicate */
  if (target_manager_find_duplicates_dev(m, dt, GATE, 4, CELL, 1, &per, 1, (int*)info_dev) != 0) { fprintf(stderr, "find: %s\n", target_manager_last_error()); return 7; }
  hipDeviceSynchronize();
  hipMemcpy(info, info_dev, sizeof info, 2); hipMemcpy(dup, dup_dev, ALL, 2); hipMemcpy(pb, pb_dev, sizeof(int) * ALL, 2);
  hipMemcpy(ps, ps_dev, sizeof(int) * ALL, 2); hipMemcpy(d2, d2_dev, sizeof(double) * ALL, 2);
  if (info[0] != TWINS || info[1] != 1 || info[2] != 1 || info[3] != 0) FAIL("info %d %d %d %d", info[0], info[1], info[2], info[3]);
  for (int i = 0; i < ALL; ++i) {
    const int paired = i < TWINS || i >= N;
    const int want_slot = i < TWINS ? N + i : (i >= N ? i - N : -1);
    if (dup[i] != (i >= N) || pb[i] != (paired ? 0 : -1) || ps[i] != want_slot) FAIL("slot %d: dup %d partner (%d, %d)", i, dup[i], pb[i], ps[i]);
    if (paired ? !(d2[i] > 0.0 && d2[i] < 1.0) : d2[i] != -1.0) FAIL("slot %d: d2 %g", i, d2[i]);
  }
  for (int k = 0; k < TWINS; ++k) if (memcmp(&d2[k], &d2[N + k], sizeof(double)) != 0) FAIL("pair %d: the partners' d2 differ", k);
  /* refusals: -1, a message, nothing changed */
  static unsigned retired[ALL], kept[ALL];
  long rinfo[4];
  if (target_manager_retire_duplicates(m, dt, GATE, 4, CELL, 1, retired, kept, TWINS - 1, rinfo) != -1 ||
      !strstr(target_manager_last_error(), "targets to retire")) FAIL("a cap too small was not refused: %s", target_manager_last_error());
  if (target_manager_find_duplicates_dev(m, dt, GATE, 4, CELL, 1, &per, 2, (int*)info_dev) != -1 ||
      !strstr(target_manager_last_error(), "n_batches")) FAIL("a wrong number of batches was not refused: %s", target_manager_last_error());
  if (target_manager_find_duplicates_dev(m, dt, GATE, 4, CELL, 256, &per, 1, (int*)info_dev) != -1 ||
      !strstr(target_manager_last_error(), "min_hits")) FAIL("min_hits 256 was not refused");
  if (target_manager_retire_duplicates(m, dt, GATE, 4, 0.0, 1, retired, kept, ALL, rinfo) != -1) FAIL("cell 0 was not refused");
  if (target_manager_size(m) != ALL) FAIL("a refused call changed the size");
  /* retire: the twins go (ascending former slot), every target keeps its id, slot and counters */
  if (target_manager_retire_duplicates(m, dt, GATE, 4, CELL, 1, retired, kept, ALL, rinfo) != 0) { fprintf(stderr, "retire: %s\n", target_manager_last_error()); return 8; }
  if (rinfo[0] != TWINS || rinfo[1] != 1 || rinfo[2] != 1 || rinfo[3] != 0) FAIL("retire info %ld %ld %ld %ld", rinfo[0], rinfo[1], rinfo[2], rinfo[3]);
  for (int k = 0; k < TWINS; ++k) if (retired[k] != 9000u + (unsigned)k || kept[k] != 100u + (unsigned)k) FAIL("pair %d: retired %u kept %u", k, retired[k], kept[k]);
  target_batch_c* b = target_manager_get_batch(m, 0);
  static unsigned slot_ids[LD];
  if (target_manager_size(m) != N || target_batch_slot_ids(b, slot_ids, LD) != N) FAIL("size after retire %ld", target_manager_size(m));
  for (int i = 0; i < N; ++i) if (slot_ids[i] != 100u + (unsigned)i) FAIL("slot %d holds %u", i, slot_ids[i]);
  int mi = -1, hi = -1;
  if (target_manager_get_track_counts(m, 101u, &mi, &hi) != 0 || mi != 0 || hi != 2) FAIL("counters of 101: %d %d", mi, hi);
  if (target_manager_get_track_counts(m, 9001u, &mi, &hi) != 1) FAIL("a retired id still has counters");
  if (target_manager_retire_duplicates(m, dt, GATE, 4, CELL, 1, NULL, NULL, 0, rinfo) != 0 || rinfo[0] != 0) FAIL("a second call found %ld", rinfo[0]);
  target_manager_delete(m);
  hipFree(has_dev); hipFree(dup_dev); hipFree(pb_dev); hipFree(ps_dev); hipFree(d2_dev); hipFree(info_dev);
  if (fail) return 1;
  printf("find duplicates test ok\n");
  return 0;
}
