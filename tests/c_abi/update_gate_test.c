/* update_gate_test.c -- a plain C caller (gcc, C99, no HIP headers) of the update policy of the by-id paths in
 * include/target_estimation_amd/target_batch_c.h: target_manager_set_update_gate, ..._get_update_gate, ..._update_gate_served and
 * target_manager_update_meas_batch_gated, around the two-call node tick of examples/node_tick.c (update by id + read-back).
 * The arithmetic is not re-derived here (tests/test_gpu_update_gate.py holds it to the masked run and to the dense calls); this
 * program checks the C calling convention and that one outlier is kept out and one lost target is re-acquired, and prints the
 * runs and events it saw.
 * usage: update_gate_test <uniform_acceleration model.yaml>   (exit code 0 = pass) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "target_batch_c.h"

#define N 40
#define TICKS 12
#define GAMMA 300.0
#define K 3
#define OUTLIER 5      /* one 0.5 m outlier on tick 4 */
#define LOST 17        /* seen 50 m away from tick 6 on */
#define UA 2           /* the model type of the yaml file */

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yaml\n", argv[0]); return 2; }
  target_manager_c* m = target_manager_new_ex(argv[1], TARGET_DTYPE_F64, 0);
  if (!m) { fprintf(stderr, "target_manager_new_ex failed: %s\n", target_manager_last_error()); return 3; }
  int fail = 0;
  const double dt = 0.004;
  static unsigned ids[N + 1];
  static double p0[N * 7];
  for (int i = 0; i < N; ++i) { ids[i] = 50u + 2u * (unsigned)(N - 1 - i); p0[i * 7] = 0.25 * i; p0[i * 7 + 6] = 1.0; }
  ids[N] = 7u;   /* an unknown id at the end of every call */

  /* the policy: refusals, then set before the targets exist (batches created later inherit it), read back */
  if (target_manager_set_update_gate(m, UA, -1.0, -1) >= 0 || !strstr(target_manager_last_error(), "gate")) { fprintf(stderr, "nis_max < 0 accepted\n"); fail = 1; }
  if (target_manager_set_update_gate(m, UA, GAMMA, 128) >= 0) { fprintf(stderr, "max_rejects 128 accepted\n"); fail = 1; }
  if (target_manager_set_update_gate(m, UA, 0.0, K) >= 0) { fprintf(stderr, "runs without a gate accepted\n"); fail = 1; }
  if (target_manager_update_gate_served(m, UA) != -1) { fprintf(stderr, "served before a batch exists\n"); fail = 1; }
  if (target_manager_set_update_gate(m, -1, GAMMA, K) != 0) { fprintf(stderr, "set_update_gate: %s\n", target_manager_last_error()); return 4; }
  double g = 0.0;
  int k = 0;
  if (target_manager_get_update_gate(m, UA, &g, &k) != 0 || g != GAMMA || k != K) { fprintf(stderr, "get_update_gate: %g %d\n", g, k); fail = 1; }
  if (target_manager_init_batch(m, ids, N, dt, 0.0, p0, NULL, NULL) != N) { fprintf(stderr, "init_batch\n"); return 4; }
  if (target_manager_update_gate_served(m, UA) != 1) { fprintf(stderr, "not served\n"); fail = 1; }

  static double meas[(N + 1) * 7], nis[N + 1], pose[(N + 1) * 7];
  static unsigned char ev[N + 1], found[N + 1];
  for (int s = 0; s < TICKS; ++s) {
    memset(meas, 0, sizeof meas);
    for (int i = 0; i <= N; ++i) {
      meas[i * 7] = (i < N ? p0[i * 7] : 0.0) + ((s == 4 && i == OUTLIER) ? 0.5 : 0.0) + ((s >= 6 && i == LOST) ? 50.0 : 0.0);
      meas[i * 7 + 6] = 1.0;
    }
    /* the node tick: update by id, read back */
    const long done = target_manager_update_meas_batch_gated(m, ids, N + 1, dt, meas, NULL, nis, ev);
    if (done != N) { fprintf(stderr, "tick %d: %ld stepped: %s\n", s, done, target_manager_last_error()); fail = 1; break; }
    if (target_manager_get_est_batch(m, ids, N + 1, pose, NULL, NULL, found) != N || found[N]) { fprintf(stderr, "tick %d: read-back\n", s); fail = 1; }
    printf("tick %2d  outlier: nis %10.3f event 0x%02x run %d   lost: nis %12.3f event 0x%02x run %d\n", s, nis[OUTLIER], ev[OUTLIER],
           target_manager_get_rejection_run(m, ids[OUTLIER]), nis[LOST], ev[LOST], target_manager_get_rejection_run(m, ids[LOST]));
    if (nis[N] != -2.0 || ev[N] != 0) { fprintf(stderr, "tick %d: the unknown id reports %g / %u\n", s, nis[N], ev[N]); fail = 1; }
    for (int i = 0; i < N; ++i) {
      unsigned want = 0;
      if (s == 4 && i == OUTLIER) want = 1;
      if (i == LOST && s >= 6) want = s == 6 ? 1 : s == 7 ? 2 : s == 8 ? (0x80u | 3u) : 0;
      if (ev[i] != want) { fprintf(stderr, "tick %d entry %d: event 0x%02x, want 0x%02x (nis %g)\n", s, i, ev[i], want, nis[i]); fail = 1; }
      if (!(nis[i] >= 0.0) || ((want != 0) != (nis[i] > GAMMA))) { fprintf(stderr, "tick %d entry %d: nis %g against event 0x%02x\n", s, i, nis[i], ev[i]); fail = 1; }
    }
    /* the outlier is not folded in; the lost target coasts, then follows the jump */
    if (s == 4 && !(pose[OUTLIER * 7] - p0[OUTLIER * 7] < 1e-6 && p0[OUTLIER * 7] - pose[OUTLIER * 7] < 1e-6)) { fprintf(stderr, "the outlier moved the estimate: %g\n", pose[OUTLIER * 7]); fail = 1; }
    if ((s == 6 || s == 7) && pose[LOST * 7] > p0[LOST * 7] + 1.0) { fprintf(stderr, "tick %d: the lost target moved before its re-initialisation\n", s); fail = 1; }
    if (s >= 8 && !(pose[LOST * 7] > p0[LOST * 7] + 49.0)) { fprintf(stderr, "tick %d: the lost target was not re-acquired: x = %g\n", s, pose[LOST * 7]); fail = 1; }
  }
  if (target_manager_get_n_measurements(m, ids[OUTLIER]) != TICKS - 1 || target_manager_get_n_measurements(m, ids[LOST]) != TICKS - K) {
    fprintf(stderr, "measurement counters: %d %d\n", target_manager_get_n_measurements(m, ids[OUTLIER]), target_manager_get_n_measurements(m, ids[LOST]));
    fail = 1;
  }
  /* the reference's own symbols run under the policy too: one more outlier through the void one-target call */
  memset(meas, 0, 7 * sizeof(double));
  meas[0] = p0[OUTLIER * 7] + 0.5; meas[6] = 1.0;
  target_manager_update_meas(m, ids[OUTLIER], dt, meas);
  if (target_manager_get_rejection_run(m, ids[OUTLIER]) != 1 || target_manager_get_n_measurements(m, ids[OUTLIER]) != TICKS - 1) { fprintf(stderr, "update_meas did not gate\n"); fail = 1; }
  /* off again */
  if (target_manager_set_update_gate(m, -1, 0.0, -1) != 0) { fprintf(stderr, "clearing the policy\n"); fail = 1; }
  target_manager_update_meas(m, ids[OUTLIER], dt, meas);
  if (target_manager_get_n_measurements(m, ids[OUTLIER]) != TICKS) { fprintf(stderr, "the cleared policy still gates\n"); fail = 1; }
  target_manager_delete(m);
  printf(fail ? "UPDATE GATE TEST FAILED\n" : "update gate test ok\n");
  return fail;
}
