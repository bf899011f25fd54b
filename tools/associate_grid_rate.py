#!/usr/bin/env python3
"""The grid form of the association against the brute-force form: how long the device forms take (Batch.associate with a CUDA frame,
cell=None and cell=0.45; GPU only).  The scenes are tools/associate_rate.py's: uniform_velocity, fp64, axis-separable targets on a
lattice of 0.25 m (S is 0.11 m per axis: with gate 16 the reach of the box is 0.447 m, so cell = 0.45 leaves every slot narrow), a
frame of nine tenths of min(N, M) detections on a target's predicted position plus 5 cm of noise, the rest clutter within 0.3 m of
some target.  HIP events around `calls` back-to-back calls after a warm call, `reps` repetitions, median and spread, rounds 1 and 4.
  (10^4, 10^4), (10^5, 10^4), (10^6, 4096): both forms in the same run, and the ratio brute / grid.
  (10^6, 10^5), (10^6, 10^6): the grid form alone (the brute-force form refuses M > 65536).
Reported per shape and form: microseconds per call and per round run (info[1]), info (info[3] = wide slots), and for the grid form
  pair_forms_round1   the pair forms the two narrow scans evaluate in the first round, counted on the CPU with the device's own cell
                      map and hash (bucket collisions included; wide slots would add theirs: none here), next to 2 N M;
The time of the binning apart from the scans is not visible from outside a call: it comes from a kernel trace of one shape in a run
of its own, the kernels' names saying which part is which (profiles/associate_grid_kernel_times.txt):
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/associate_grid_rate.py --only 1e6,1e5 --rounds 1 --reps 2 --calls 5
Nothing is gated.   python tools/associate_grid_rate.py --out profiles/associate_grid_rate.json [--reps 5] [--calls 10] [--scale s]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = [(10_000, 10_000), (100_000, 10_000), (1_000_000, 4096)]
GRID_ONLY = [(1_000_000, 100_000), (1_000_000, 1_000_000)]
DT, GATE, NOISE, SPACING, CELL = 0.004, 16.0, 0.05, 0.25, 0.45


def _coord(np, x, cell):
    q = np.floor(x / cell)
    return np.clip(q, -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def _bucket(np, c, H):
    m = np.uint64(0xffffffff)
    u = lambda v: v.astype(np.uint64) & m
    h = ((u(c[:, 0]) * np.uint64(0x9E3779B1)) & m) ^ ((u(c[:, 1]) * np.uint64(0x85EBCA77)) & m) ^ ((u(c[:, 2]) * np.uint64(0xC2B2AE3D)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(13)
    return (h & np.uint64(H - 1)).astype(np.int64)


def _buckets(count):
    h = 1024
    while h < 2 * count:
        h *= 2
    return h


def _forms_round1(np, zhat, det, cell):
    """what the first round's two narrow scans evaluate: per row the entries of the detection buckets of its 27 cells, per detection
    the entries of the row buckets of its 27 cells"""
    total = 0
    for own, other in ((zhat, det), (det, zhat)):
        H = _buckets(len(other))
        counts = np.bincount(_bucket(np, _coord(np, other, cell), H), minlength=H)
        c = _coord(np, own, cell)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    total += int(counts[_bucket(np, c + np.array([dx, dy, dz]), H)].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the shapes (a trial run of the tool itself)")
    ap.add_argument("--only", default=None, help="N,M: that shape alone, the grid form alone, no pair-form count -- the run to put under a "
                                                 "kernel trace (rocprofv3 --kernel-trace --stats -- python tools/associate_grid_rate.py --only "
                                                 "1e6,1e5 --rounds 1), whose per-kernel times separate table, binning, scans and outputs")
    ap.add_argument("--rounds", default="1,4", help="the round counts to time")
    args = ap.parse_args()
    rounds_list = [int(r) for r in args.rounds.split(",")]
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("associate_grid_rate: needs a GPU")
    import target_estimation_amd as te
    record = {"tool": "tools/associate_grid_rate.py", "device": torch.cuda.get_device_name(0), "gate": GATE, "cell": CELL,
              "note": "times in microseconds; every number here was measured by this run", "shapes": []}

    def timed(b, det, rounds, cell):
        out = b.associate(det, DT, gate=GATE, rounds=rounds, cell=cell)          # the warm call
        torch.cuda.synchronize()
        info = out.info.cpu().numpy().tolist()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                b.associate(det, DT, gate=GATE, rounds=rounds, out=out, cell=cell)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / args.calls)
        med = statistics.median(times)
        return dict(info=info, call_us=times, call_us_median=med, spread=(max(times) - min(times)) / med, us_per_round_run=med / max(info[1], 1)), out

    shapes = BOTH + GRID_ONLY
    if args.only:
        shapes = [tuple(int(float(v)) for v in args.only.split(","))]
    for N, M in shapes:
        both = (N, M) in BOTH and not args.only
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
        det = det[rng.permutation(M)]
        forms1 = None if args.only else _forms_round1(np, p0[:, :3] + v0[:, :3] * DT, det[:, :3], CELL)
        det = torch.from_numpy(det).cuda()
        row = dict(N=N, M=M, pair_forms_round1=forms1, pair_forms_brute_round=2 * N * M, rounds={})
        for rounds in rounds_list:
            entry = {}
            g, og = timed(b, det, rounds, CELL)
            entry["grid"] = g
            if both:
                br, ob = timed(b, det, rounds, None)
                entry["brute"] = br
                entry["brute_over_grid"] = br["call_us_median"] / g["call_us_median"]
                torch.cuda.synchronize()
                same = all(torch.equal(x, y) for x, y in ((og.slot_of_det, ob.slot_of_det), (og.det_of_slot, ob.det_of_slot),
                                                           (og.d2_of_det, ob.d2_of_det), (og.info[:3], ob.info[:3])))
                entry["same_result_as_brute"] = bool(same)
            row["rounds"][str(rounds)] = entry
        record["shapes"].append(row)
        brief = dict(N=N, M=M, forms1=forms1)
        for r, e in row["rounds"].items():
            brief["grid_us_r" + r] = round(e["grid"]["call_us_median"], 1)
            brief["info_r" + r] = e["grid"]["info"]
            if "brute" in e:
                brief["brute_us_r" + r] = round(e["brute"]["call_us_median"], 1)
                brief["ratio_r" + r] = round(e["brute_over_grid"], 2)
                brief["same_r" + r] = e["same_result_as_brute"]
        print(json.dumps(brief), flush=True)
        mgr.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
