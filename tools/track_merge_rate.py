#!/usr/bin/env python3
"""How long the duplicate-track search takes (TargetManager.find_duplicates / retire_duplicates; GPU only).
Scenes: tools/associate_grid_rate.py's lattice (uniform_velocity, fp64, axis-separable, Sigma about 0.1 m per axis, gate 16; the
reach of a row's box is sqrt(16 * 2 Sigma (1 + 2^-10)) = 0.566 m, so cell = 0.57 leaves nothing wide); one target in a hundred is
given a twin 5 cm away; min_hits = 0, so every row is eligible.  N = 10^4, 10^5, 10^6 (twins included), rounds 1 and 4.
  "sparse"  spacing 0.6 m, above the pair reach: only the twins pair -- the case the call is for.
  "dense"   spacing 0.25 m, the association tool's own: the lattice neighbours are inside the pair gate too (d2 = 3.1), so most
            rows pair -- the walk's worst case, and the scene the association's figures of DESIGN 3.19 come from.
  find_duplicates    HIP events around `calls` back-to-back calls after a warm one, `reps` repetitions: median and spread.
  retire_duplicates  one call per shape by wall clock (it waits on the host by design) on a manager of its own.
  yardstick          Batch.associate(cell=0.45) of the same N targets against M = N detections, one round, in the same process:
                     the self-join does one walk per round where the association does two, with about twice the arithmetic a visit.
  bytes              what the host-composed path would read back (get_state: x and P of every target) next to what
                     retire_duplicates moves across the bus (the counts, info, and three ints per retired target); computed from
                     the shapes, not measured.  There is no parent path to beat: no speed-up is reported.
A kernel trace of one shape goes in a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/track_merge_rate.py --scenes dense --only 1e6 --rounds 1 --reps 2 --calls 5 --no-retire
Nothing is gated.   python tools/track_merge_rate.py --out profiles/track_merge_rate.json [--reps 5] [--calls 10] [--scale s]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [10_000, 100_000, 1_000_000]
DT, GATE, CELL, ASSOC_CELL, NOISE, TWIN = 0.004, 16.0, 0.57, 0.45, 0.05, 0.05
SCENES = {"sparse": 0.6, "dense": 0.25}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the shapes (a trial run of the tool itself)")
    ap.add_argument("--only", default=None, help="N: that shape alone, find_duplicates alone")
    ap.add_argument("--rounds", default="1,4")
    ap.add_argument("--scenes", default="sparse,dense")
    ap.add_argument("--no-retire", action="store_true")
    args = ap.parse_args()
    rounds_list = [int(r) for r in args.rounds.split(",")]
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_merge_rate: needs a GPU")
    import target_estimation_amd as te
    record = {"tool": "tools/track_merge_rate.py", "device": torch.cuda.get_device_name(0), "gate": GATE, "cell": CELL, "min_hits": 0,
              "note": "times in microseconds; every time here was measured by this run; bytes are computed from the shapes", "shapes": []}

    def world(N, SPACING):
        rng = np.random.default_rng(N)
        base = N - N // 101                      # one twin per hundred targets
        i = np.arange(base)
        p0 = np.zeros((N, 7)); p0[:, 6] = 1.0
        p0[:base, 0], p0[:base, 1], p0[:base, 2] = SPACING * (i % 100), SPACING * ((i // 100) % 100), SPACING * (i // 10000)
        v0 = np.zeros((N, 6)); v0[:base, :3] = rng.uniform(-1, 1, (base, 3))
        own = rng.permutation(base)[:N - base]
        u = rng.normal(size=(N - base, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        p0[base:, :3] = p0[own, :3] + TWIN * u
        v0[base:] = v0[own]
        mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        Q, R, P0 = 1e-6 * np.eye(6), 2.5e-3 * np.eye(3), 1e-2 * np.eye(6)
        assert mgr.init_batch(np.arange(N, dtype=np.uint32), DT, 0.0, p0, v0, None, type=te.MODEL_TYPES["uniform_velocity"], Q=Q, R=R, P0=P0) == N
        return mgr, p0, v0, rng

    def events(call):
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / args.calls)
        med = statistics.median(times)
        return dict(call_us=times, call_us_median=med, spread=(max(times) - min(times)) / med)

    sizes = [int(float(args.only))] if args.only else SIZES
    for scene, N in [(sc, n) for sc in args.scenes.split(",") for n in sizes]:
        N = max(int(N * args.scale), 202)
        mgr, p0, v0, rng = world(N, SCENES[scene])
        row = dict(scene=scene, spacing=SCENES[scene], N=N, twins=N // 101, rounds={})
        for rounds in rounds_list:
            out = mgr.find_duplicates(DT, GATE, CELL, rounds=rounds, min_hits=0)          # the warm call
            torch.cuda.synchronize()
            e = events(lambda: mgr.find_duplicates(DT, GATE, CELL, rounds=rounds, min_hits=0, out=out))
            e["info"] = out.info.cpu().numpy().tolist()
            row["rounds"][str(rounds)] = e
        if not args.only:
            # the yardstick: the association's grid form at M = N, one round
            M = N
            det = np.zeros((M, 7)); det[:, 6] = 1.0
            det[:, :3] = (p0[:, :3] + v0[:, :3] * DT + rng.normal(0, NOISE, (N, 3)))[rng.permutation(N)]
            det = torch.from_numpy(det).cuda()
            b = mgr.batches()[0]
            aout = b.associate(det, DT, gate=GATE, rounds=1, cell=ASSOC_CELL)
            torch.cuda.synchronize()
            a = events(lambda: b.associate(det, DT, gate=GATE, rounds=1, out=aout, cell=ASSOC_CELL))
            a["info"] = aout.info.cpu().numpy().tolist()
            row["associate_grid_M_eq_N_round1"] = a
            row["find_round1_over_associate"] = row["rounds"][str(rounds_list[0])]["call_us_median"] / a["call_us_median"]
        if not args.only and not args.no_retire:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = mgr.retire_duplicates(DT, GATE, CELL, rounds=4, min_hits=0)
            wall = time.perf_counter() - t0
            row["retire_duplicates"] = dict(wall_us=wall * 1e6, retired=int(r.retired), rounds_run=int(r.rounds_run), settled=int(r.settled),
                                            wide=int(r.wide), size_after=int(mgr.size()))
            row["bytes"] = dict(host_path_get_state=N * (6 + 36) * 8, device_path_readback=(1 + 4) * 4 + int(r.retired) * 12)
        record["shapes"].append(row)
        brief = dict(scene=scene, N=N)
        for rr, e in row["rounds"].items():
            brief["find_us_r" + rr] = round(e["call_us_median"], 1)
            brief["spread_r" + rr] = round(e["spread"], 3)
            brief["info_r" + rr] = e["info"]
        if "associate_grid_M_eq_N_round1" in row:
            brief["assoc_us"] = round(row["associate_grid_M_eq_N_round1"]["call_us_median"], 1)
            brief["find_over_assoc"] = round(row["find_round1_over_associate"], 3)
        if "retire_duplicates" in row:
            brief["retire"] = row["retire_duplicates"]
            brief["bytes"] = row["bytes"]
        print(json.dumps(brief), flush=True)
        mgr.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
