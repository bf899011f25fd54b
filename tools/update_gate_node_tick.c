/* update_gate_node_tick.c -- the node tick (target_manager_update_meas_batch + target_manager_get_est_batch, ids in any order) from
 * plain C, timed with a host clock around the two calls (the second one ends in the flush's completion), without and with the
 * update policy of target_manager_set_update_gate (gamma = 300, K = 3) on a clean stream: what profiles/r13_update_gate.json
 * records.  The forms run on managers of their own in the same process, alternated in blocks of BLOCK ticks until each has run
 * for at least a second; per form the median over its blocks' median tick and the spread (largest - smallest block median).
 * Built without -DWITH_POLICY it runs the no-policy form alone, twice, against a library that does not have the symbols (the
 * parent commit).
 *   gcc -std=c99 -O2 [-DWITH_POLICY] -I include/target_estimation_amd tools/update_gate_node_tick.c -o node_tick_gate \
 *       -L target_estimation_amd/lib -ltarget_estimation_amd -lm -Wl,-rpath,$PWD/target_estimation_amd/lib
 *   ./node_tick_gate models/model_angular_rates_params.yaml 300        -> one JSON line */
#define _POSIX_C_SOURCE 199309L
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "target_batch_c.h"
#include "target_manager_c.h"

#define BLOCK 200
#define MAX_BLOCKS 4096

static double now_us(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}
static int cmp(const void* a, const void* b) { const double x = *(const double*)a, y = *(const double*)b; return x < y ? -1 : x > y; }
static double median(double* v, int n) { qsort(v, (size_t)n, sizeof(double), cmp); return n & 1 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]); }

static void measurement(unsigned id, long tick, double* m) {
  const double w = 0.3 + 0.01 * (double)(id % 17), r = 1.0 + 0.05 * (double)(id % 5), t = 0.004 * (double)tick;
  unsigned s = id * 2654435761u + (unsigned)tick * 40503u;
  double noise[3];
  int k;
  for (k = 0; k < 3; ++k) { s = s * 1664525u + 1013904223u; noise[k] = 1e-3 * ((double)(s >> 8) / 16777216.0 - 0.5); }
  m[0] = r * cos(w * t) + noise[0]; m[1] = r * sin(w * t) + noise[1]; m[2] = 0.1 * (double)(id % 3) + noise[2];
  m[3] = 0.0; m[4] = 0.0; m[5] = sin(0.5 * w * t); m[6] = cos(0.5 * w * t);
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s model.yaml n_ids\n", argv[0]); return 2; }
  const long n = atol(argv[2]);
  const double dt = 0.004;
  if (n < 1 || n > 1024) { fprintf(stderr, "1 .. 1024 ids\n"); return 2; }
  target_manager_c* mgr[2] = {target_manager_new(argv[1]), target_manager_new(argv[1])};
  if (!mgr[0] || !mgr[1]) { fprintf(stderr, "no manager\n"); return 3; }
  unsigned* ids = (unsigned*)malloc(sizeof(unsigned) * (size_t)n);
  double* meas = (double*)malloc(sizeof(double) * 7 * (size_t)n);
  double* pose = (double*)malloc(sizeof(double) * 7 * (size_t)n);
  unsigned char* has = (unsigned char*)malloc((size_t)n);
  unsigned char* found = (unsigned char*)malloc((size_t)n);
  long i;
  for (i = 0; i < n; ++i) { ids[i] = 100u + 7u * (unsigned)((i * 37) % n); measurement(ids[i], 0, meas + 7 * i); }
#ifdef WITH_POLICY
  if (target_manager_set_update_gate(mgr[1], -1, 300.0, 3) != 0) { fprintf(stderr, "%s\n", target_manager_last_error()); return 4; }
#endif
  int f;
  for (f = 0; f < 2; ++f)
    if (target_manager_init_batch(mgr[f], ids, n, dt, 0.0, meas, NULL, NULL) != n) return 4;
  static double blocks[2][MAX_BLOCKS], tick_us[BLOCK];
  double spent[2] = {0.0, 0.0};
  int nb[2] = {0, 0};
  long tick[2] = {0, 0};
  while ((spent[0] < 1.2e6 || spent[1] < 1.2e6) && nb[0] < MAX_BLOCKS) {
    for (f = 0; f < 2; ++f) {
      int s;
      for (s = 0; s < BLOCK; ++s) {
        ++tick[f];
        for (i = 0; i < n; ++i) {
          measurement(ids[i], tick[f], meas + 7 * i);
          has[i] = (unsigned char)(((ids[i] + 3u * (unsigned)tick[f]) % 10u) != 0u);
        }
        const double t0 = now_us();
        const long stepped = target_manager_update_meas_batch(mgr[f], ids, n, dt, meas, has);
        const long read = target_manager_get_est_batch(mgr[f], ids, n, pose, NULL, NULL, found);
        tick_us[s] = now_us() - t0;
        if (stepped != n || read != n) { fprintf(stderr, "tick failed: %s\n", target_manager_last_error()); return 5; }
        spent[f] += tick_us[s];
      }
      blocks[f][nb[f]++] = median(tick_us, BLOCK);
    }
  }
  long rejected = 0;
  for (i = 0; i < n; ++i) rejected += target_manager_get_n_measurements(mgr[0], ids[i]) - target_manager_get_n_measurements(mgr[1], ids[i]);
  double out[2][2];
  for (f = 0; f < 2; ++f) {   /* (the first block of a form warms up: left out) */
    double* b = blocks[f] + 1;
    const int k = nb[f] - 1;
    qsort(b, (size_t)k, sizeof(double), cmp);
    out[f][1] = b[k - 1] - b[0];
    out[f][0] = median(b, k);
  }
#ifdef WITH_POLICY
  const char* second = "policy";
#else
  const char* second = "no_policy_again";
#endif
  printf("{\"model\": \"%s\", \"ids\": %ld, \"block_ticks\": %d, \"blocks\": %d, \"no_policy\": {\"median_us\": %.3f, \"spread_us\": %.3f}, "
         "\"%s\": {\"median_us\": %.3f, \"spread_us\": %.3f}, \"measurements_rejected_by_second_form\": %ld}\n",
         argv[1], n, BLOCK, nb[0] - 1, out[0][0], out[0][1], second, out[1][0], out[1][1], rejected);
  target_manager_delete(mgr[0]);
  target_manager_delete(mgr[1]);
  return 0;
}
