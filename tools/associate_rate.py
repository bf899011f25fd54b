#!/usr/bin/env python3
"""Association of unlabelled detections: how long the device form takes (Batch.associate with a CUDA frame; GPU only).
Shapes (N targets, M detections): (10^4, 10^4), (10^5, 10^4), (10^6, 4096), each with 1 and 4 rounds.  Targets: uniform_velocity,
fp64, axis-separable, on a lattice of 0.25 m (S is 0.11 m per axis, so with gate 16 a target's neighbours are inside its gate: a
contested scene that needs several rounds); the frame: nine tenths of min(N, M) detections on a target's predicted position plus
5 cm of noise, the rest clutter within 0.3 m of some target.  HIP events around `calls` back-to-back calls after a warm-up call
(which also sizes the scratch), `reps` repetitions; the record keeps every repetition, the median and the spread ((max - min) / median).
Reported per shape: microseconds per call and per round actually run (info[1]), pair forms per second -- a round evaluates d^2 for
every (target, detection) pair twice, once per scan orientation, 2 N M forms, less what matched rows and columns skip, which is NOT
subtracted -- and the share of the fp64 vector peak that the forms' 23 flops each imply (78.6 TFLOP/s, the public figure for the
part: an upper bound the scans cannot reach, since plain multiplies and adds count one flop per instruction where the peak counts
an fma as two).  There is no parent to compare a new call with: the numbers are reported, not gated.
  python tools/associate_rate.py --out profiles/associate_rate.json [--reps 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(10_000, 10_000), (100_000, 10_000), (1_000_000, 4096)]
ROUNDS = [1, 4]
DT, GATE, NOISE, SPACING = 0.004, 16.0, 0.05, 0.25
FLOPS_PER_FORM = 23            # assoc_d2: 3 subtractions, 12 multiplies, 8 additions
FP64_VECTOR_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the shapes (a trial run of the tool itself)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("associate_rate: needs a GPU")
    import target_estimation_amd as te
    record = {"tool": "tools/associate_rate.py", "device": torch.cuda.get_device_name(0), "gate": GATE, "flops_per_pair_form": FLOPS_PER_FORM,
              "fp64_vector_peak_assumed": FP64_VECTOR_PEAK, "note": "times in microseconds; every number here was measured by this run", "shapes": []}
    for N, M in SHAPES:
        N, M = max(int(N * args.scale), 1), max(int(M * args.scale), 1)
        rng = np.random.default_rng(N + M)
        mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        i = np.arange(N)
        p0 = np.zeros((N, 7)); p0[:, 6] = 1.0
        p0[:, 0], p0[:, 1], p0[:, 2] = SPACING * (i % 100), SPACING * ((i // 100) % 100), SPACING * (i // 10000)
        v0 = np.zeros((N, 6)); v0[:, :3] = rng.uniform(-1, 1, (N, 3))
        Q, R, P0 = 1e-6 * np.eye(6), 2.5e-3 * np.eye(3), 1e-2 * np.eye(6)
        assert mgr.init_batch(np.arange(N, dtype=np.uint32), DT, 0.0, p0, v0, None, type=te.MODEL_TYPES["uniform_velocity"], Q=Q, R=R, P0=P0) == N
        b = mgr.batches()[0]
        det = np.zeros((M, 7)); det[:, 6] = 1.0
        k = min(N, M) * 9 // 10
        own = rng.permutation(N)[:k]
        det[:k, :3] = p0[own, :3] + v0[own, :3] * DT + rng.normal(0, NOISE, (k, 3))
        det[k:, :3] = p0[rng.integers(0, N, M - k), :3] + rng.uniform(-0.3, 0.3, (M - k, 3))
        det = torch.from_numpy(det[rng.permutation(M)]).cuda()
        for rounds in ROUNDS:
            out = b.associate(det, DT, gate=GATE, rounds=rounds)          # the warm call
            torch.cuda.synchronize()
            info = out.info.cpu().numpy().tolist()
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    b.associate(det, DT, gate=GATE, rounds=rounds, out=out)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / args.calls)
            med = statistics.median(times)
            run = max(info[1], 1)
            forms = 2.0 * N * M * run
            row = dict(N=N, M=M, rounds_asked=rounds, info=info, call_us=times, call_us_median=med, spread=(max(times) - min(times)) / med,
                       us_per_round_run=med / run, pair_forms_per_s=forms / (med * 1e-6),
                       share_of_fp64_vector_peak=forms * FLOPS_PER_FORM / (med * 1e-6) / FP64_VECTOR_PEAK)
            record["shapes"].append(row)
            print(json.dumps({k2: (round(v, 5) if isinstance(v, float) else v) for k2, v in row.items() if k2 != "call_us"}), flush=True)
        mgr.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
