/* lifecycle_test.c -- a plain C caller (gcc, C99, no HIP headers) of the track lifecycle in
 * include/target_estimation_amd/target_batch_c.h: target_manager_lifecycle, target_batch_track_counts and
 * target_manager_get_track_counts, behind target_manager_associate_grid_dev and target_manager_step_sequence_all(n_ticks = 1).
 * The program checks the calling convention itself: N targets 4 m apart, a frame that sees all but the first three and holds five
 * new objects (one of them with a NaN), so who is retired, who is born, with which ids and in which slots is known.
 * Device buffers come from the HIP runtime the library links, declared by hand.
 * usage: lifecycle_test <uniform_velocity model.yaml>   (exit code 0 = pass) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

extern int hipMalloc(void** p, size_t bytes);
extern int hipFree(void* p);
extern int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);   /* 1: host to device, 2: device to host */
extern int hipDeviceSynchronize(void);

#define N 70
#define GONE 3     /* targets 0..2 are not seen */
#define NEW 5      /* new objects; the second one has a NaN */
#define MM (N - GONE + NEW)
#define LD 128
#define GATE 9.0

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); fail = 1; } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ids[N];
  static double p0[N * 7];
  for (int i = 0; i < N; ++i) { ids[i] = 100u + (unsigned)i; p0[i * 7] = 4.0 * i; p0[i * 7 + 6] = 1.0; }
  target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
  if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
  if (target_manager_init_batch(m, ids, N, dt, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "init_batch\n"); return 4; }
  /* the frame: targets N-1 .. GONE (reversed), then the new objects at y = 50 */
  static double det[MM * 7];
  for (int j = 0; j < MM; ++j) {
    double* d = det + j * 7;
    d[6] = 1.0;
    if (j < N - GONE) d[0] = 4.0 * (N - 1 - j) + 0.001;
    else { d[0] = 4.0 * (j - (N - GONE)); d[1] = 50.0; }
  }
  det[(N - GONE + 1) * 7 + 2] = NAN;
  void *det_dev = NULL, *meas_dev = NULL, *has_dev = NULL, *sod_dev = NULL, *info_dev = NULL;
  if (hipMalloc(&det_dev, sizeof det) || hipMalloc(&meas_dev, sizeof(double) * 7 * LD) || hipMalloc(&has_dev, LD) ||
      hipMalloc(&sod_dev, sizeof(int) * MM) || hipMalloc(&info_dev, sizeof(int) * 4)) { fprintf(stderr, "hipMalloc\n"); return 5; }
  hipMemcpy(det_dev, det, sizeof det, 1);
  target_assoc_out_c per;
  memset(&per, 0, sizeof per);
  per.meas_out_dev = meas_dev; per.ld = LD; per.has_meas_out_dev = (unsigned char*)has_dev;
  target_batch_sequence_c seq;
  memset(&seq, 0, sizeof seq);
  seq.meas_dev = meas_dev; seq.tick_stride = 7 * LD; seq.ld = LD; seq.has_meas_dev = (const unsigned char*)has_dev; seq.has_stride = LD;
  const unsigned char* masks[1] = {(const unsigned char*)has_dev};
  target_lifecycle_c pol;
  memset(&pol, 0, sizeof pol);
  pol.max_misses = 2; pol.birth_type = TARGET_UNIFORM_VELOCITY; pol.first_id = 9000u; pol.max_births = 3; pol.dt0 = dt; pol.t_birth = dt;
  static unsigned retired[N];
  long info[6];
  static unsigned char miss[LD], hits[LD];
  static unsigned slot_ids[LD];
  target_batch_c* b = target_manager_get_batch(m, 0);

  for (int frame = 0; frame < 2; ++frame) {
    if (target_manager_associate_grid_dev(m, dt, (const double*)det_dev, MM, GATE, 4, 2.0, &per, 1, (int*)sod_dev, NULL, NULL, (int*)info_dev) != 0) {
      fprintf(stderr, "associate_grid_dev: %s\n", target_manager_last_error()); return 6; }
    if (target_manager_step_sequence_all(m, 1, dt, &seq, 1, 0, NULL, 0.0, 0) != 0) { fprintf(stderr, "step: %s\n", target_manager_last_error()); return 6; }
    pol.first_id = 9000u + 100u * (unsigned)frame;
    memset(info, 0xff, sizeof info);
    if (target_manager_lifecycle(m, (const double*)det_dev, (const int*)sod_dev, MM, masks, 1, &pol, retired, N, info) != 0) {
      fprintf(stderr, "lifecycle: %s\n", target_manager_last_error()); return 7; }
    if (frame == 0) {
      /* nobody is stale after one miss; four finite unmatched rows, three born under the cap, one non-finite */
      if (info[0] != 0 || info[1] != 3 || info[2] != 1 || info[3] != 1 || info[4] != 9000 || info[5] != 9003)
        FAIL("frame 0 info %ld %ld %ld %ld %ld %ld", info[0], info[1], info[2], info[3], info[4], info[5]);
      if (target_manager_size(m) != N + 3 || target_batch_size(b) != N + 3) FAIL("frame 0 size %ld", target_manager_size(m));
      if (target_batch_track_counts(b, miss, hits) != 0) FAIL("track_counts: %s", target_manager_last_error());
      for (int i = 0; i < N + 3; ++i) {
        const int want_miss = i < GONE ? 1 : 0, want_hits = (i >= GONE && i < N) ? 1 : 0;
        if (miss[i] != want_miss || hits[i] != want_hits) FAIL("frame 0 slot %d: miss %d hits %d", i, miss[i], hits[i]);
      }
    } else {
      /* the second miss retires 100, 101, 102 (ascending former slot); the survivors from the tail fill slots 0..2; the three
       * targets born in frame 0 sit on their detections and are matched; the capped row of frame 0 is born now */
      if (info[0] != GONE || info[1] != 1 || info[2] != 0 || info[3] != 1 || info[4] != 9100 || info[5] != 9101)
        FAIL("frame 1 info %ld %ld %ld %ld %ld %ld", info[0], info[1], info[2], info[3], info[4], info[5]);
      for (int k = 0; k < GONE; ++k) if (retired[k] != 100u + (unsigned)k) FAIL("retired[%d] = %u", k, retired[k]);
      if (target_manager_size(m) != N + 1) FAIL("frame 1 size %ld", target_manager_size(m));
      if (target_batch_slot_ids(b, slot_ids, LD) != N + 1) FAIL("slot_ids");
      /* before: slots 0..69 = ids 100..169, 70..72 = 9000..9002.  new size 70: holes 0, 1, 2 <- slots 70, 71, 72; then 9100 at slot 70 */
      for (int k = 0; k < GONE; ++k) if (slot_ids[k] != 9000u + (unsigned)k) FAIL("slot %d holds %u", k, slot_ids[k]);
      if (slot_ids[GONE] != 100u + GONE || slot_ids[N - 1] != 100u + N - 1 || slot_ids[N] != 9100u) FAIL("slots %u %u %u", slot_ids[GONE], slot_ids[N - 1], slot_ids[N]);
      int mi = -1, hi = -1;
      if (target_manager_get_track_counts(m, 9001u, &mi, &hi) != 0 || mi != 0 || hi != 1) FAIL("counters of 9001: %d %d", mi, hi);
      if (target_manager_get_track_counts(m, 150u, &mi, &hi) != 0 || mi != 0 || hi != 2) FAIL("counters of 150: %d %d", mi, hi);
      if (target_manager_get_track_counts(m, 9100u, &mi, &hi) != 0 || mi != 0 || hi != 0) FAIL("counters of 9100: %d %d", mi, hi);
      if (target_manager_get_track_counts(m, 100u, &mi, &hi) != 1) FAIL("a retired id still has counters");
      double pose[7];
      if (!target_manager_get_est_pose(m, 9100u, pose) || pose[0] != det[(N - GONE + 4) * 7] || pose[1] != 50.0) FAIL("pose of 9100: %g %g", pose[0], pose[1]);
    }
  }
  /* refusals: -1, a message, nothing changed */
  {
    const long size = target_manager_size(m);
    int mi = -1, hi = -1;
    /* the frame's one unmatched finite row would be born as 9000, which exists: found only after the plan has been formed */
    pol.first_id = 9000u;
    if (target_manager_lifecycle(m, (const double*)det_dev, (const int*)sod_dev, MM, masks, 1, &pol, retired, N, info) != -1 ||
        !strstr(target_manager_last_error(), "exists already")) FAIL("an id collision was not refused: %s", target_manager_last_error());
    if (target_manager_get_track_counts(m, 9001u, &mi, &hi) != 0 || mi != 0 || hi != 1) FAIL("a refused call changed the counters of 9001: %d %d", mi, hi);
    if (target_manager_lifecycle(m, (const double*)det_dev, (const int*)sod_dev, MM, masks, 2, &pol, retired, N, info) != -1 ||
        !strstr(target_manager_last_error(), "n_batches")) FAIL("a wrong number of batches was not refused: %s", target_manager_last_error());
    pol.max_misses = 300;
    if (target_manager_lifecycle(m, (const double*)det_dev, (const int*)sod_dev, MM, masks, 1, &pol, retired, N, info) != -1 ||
        !strstr(target_manager_last_error(), "max_misses")) FAIL("max_misses 300 was not refused");
    if (target_manager_lifecycle(m, (const double*)det_dev, (const int*)sod_dev, MM, masks, 1, NULL, retired, N, info) != -1) FAIL("a NULL policy was not refused");
    if (target_manager_size(m) != size) FAIL("a refused call changed the size");
  }
  target_manager_delete(m);
  hipFree(det_dev); hipFree(meas_dev); hipFree(has_dev); hipFree(sod_dev); hipFree(info_dev);
  if (fail) return 1;
  printf("lifecycle test ok\n");
  return 0;
}
