/* sharded_drop_in_test.c -- the reference's ten C symbols driving several targets, plus ONE call of
 * target_manager_set_devices: the same program on a manager spread over shards.  Run with "plain" and with a
 * device list ("0,0" = two shards on device 0); tests/test_gpu_shards.py compares the two outputs.
 * usage: sharded_drop_in_test <model.yaml> plain|<d0,d1,...>   (exit code 0 = pass) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

static double noise(unsigned* s) {   /* small deterministic zero-mean noise, sigma ~ 0.01 */
  double acc = 0.0;
  for (int k = 0; k < 12; ++k) {
    *s = *s * 1664525u + 1013904223u;
    acc += (double)(*s >> 8) / 16777216.0;
  }
  return (acc - 6.0) * 0.01;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s model.yaml plain|d0,d1,...\n", argv[0]); return 2; }
  target_manager_c* m = target_manager_new(argv[1]);
  if (!m) { fprintf(stderr, "target_manager_new failed\n"); return 3; }
  if (strcmp(argv[2], "plain") != 0) {
    int devs[16], n = 0;
    for (char* p = argv[2]; *p && n < 16;) { devs[n++] = (int)strtol(p, &p, 10); if (*p == ',') ++p; }
    if (target_manager_set_devices(m, devs, n) != 0) { fprintf(stderr, "set_devices: %s\n", target_manager_last_error()); return 4; }
  }
  enum { NT = 6 };
  const unsigned ids[NT] = {7u, 3u, 11u, 5u, 42u, 8u};
  const int n_points = 500;
  const double dt = 1.0 / 250.0;
  double p0[7] = {0, 0, 0, 0, 0, 0, 1}, meas[7] = {0, 0, 0, 0, 0, 0, 1}, pose[7], twist[6], acc[6];
  unsigned seed = 12345u;
  for (int k = 0; k < NT; ++k) { p0[0] = 0.1 * k; target_manager_init(m, ids[k], dt, p0, 0.0); }
  target_manager_init(m, 7u, dt, p0, 0.0);            /* duplicate: message, no change */
  for (int i = 0; i < n_points; ++i)
    for (int k = 0; k < NT; ++k) {
      for (int c = 0; c < 3; ++c) meas[c] = 0.1 * k * (c == 0) + (0.2 + 0.05 * c) * (double)i / n_points + noise(&seed);
      if ((i + k) % 7 == 3) target_manager_update(m, ids[k], dt);   /* predict only */
      else target_manager_update_meas(m, ids[k], dt, meas);
    }
  int fail = 0;
  for (int k = 0; k < NT; ++k) {
    if (!target_manager_get_est_pose(m, ids[k], pose) || !target_manager_get_est_twist(m, ids[k], twist) ||
        !target_manager_get_est_acceleration(m, ids[k], acc)) { fprintf(stderr, "getter %u\n", ids[k]); fail = 1; continue; }
    printf("id %u n %d pose", ids[k], target_manager_get_n_measurements(m, ids[k]));
    for (int c = 0; c < 7; ++c) printf(" %.17g", pose[c]);
    printf(" twist");
    for (int c = 0; c < 6; ++c) printf(" %.17g", twist[c]);
    printf(" acc");
    for (int c = 0; c < 6; ++c) printf(" %.17g", acc[c]);
    printf("\n");
  }
  if (target_manager_get_est_pose(m, 9u, pose)) { fprintf(stderr, "unknown id returned true\n"); fail = 1; }
  target_manager_update_meas(m, 9u, dt, meas);        /* unknown id: message only */
  target_manager_log(m);
  target_manager_delete(m);
  printf(fail ? "SHARDED DROP-IN TEST FAILED\n" : "sharded drop-in test ok\n");
  return fail;
}
