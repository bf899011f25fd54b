#!/usr/bin/env python3
"""Per-tick innovation / NIS streams at the large mixed configurations (GPU only).  For cfg4_1gpu (500 000 angular-rates + 500 000
angular-velocities, fp64) and cfg4_4m (2 000 000 + 2 000 000) -- the sizes of profiles/r05_pose_stream.json -- it times three forms
of the node's loop, eager target_manager_step_sequence_all ticks over a measurement ring:
  (a) plain   the population tick alone
  (n) nis     the population tick with a NIS-only stream per batch (target_manager_step_sequence_all_innov, one row overwritten)
  (f) full    the same with NIS and the innovations (one row and one [6][ld] block per batch, overwritten every tick)
HIP events around each timed region, a warm-up per form, forms alternated and repeated (--reps): the record has every
repetition, the median and the spread.  The expectation the record sets the measured ratios against is the ratio of algorithmic
bytes: 872 B per target per tick for the state and measurements (bench.py's figure for these populations), + 8 B of NIS in (n),
+ 8 + 48 B in (f) -- as far as the kernels are HBM-bound.  (A tick with an innovation stream runs in place; the plain eager tick
of a population beyond TE_PINGPONG_MIN_MB is an A -> B tick, so cfg4_4m also compares the two tick variants.)
--forms a --root <tree> times the plain tick of another checkout of the project (its package and built library) with this same
tool: the comparison against the parent commit.
  python tools/innov_stream_rate.py --out profiles/r09_innov_stream.json [--seconds 1.0] [--reps 3] [--configs cfg4_1gpu,cfg4_4m]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"cfg4_1gpu": [("angular_rates", 500_000), ("angular_velocities", 500_000)],
           "cfg4_4m": [("angular_rates", 2_000_000), ("angular_velocities", 2_000_000)]}
STATE_B, NIS_B, INNOV_B, PEAK = 872, 8, 48, 8.0e12
BYTES = {"a": STATE_B, "n": STATE_B + NIS_B, "f": STATE_B + NIS_B + INNOV_B}
RING, DT, SEED = 16, 0.004, 20240004


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="cfg4_1gpu,cfg4_4m")
    ap.add_argument("--forms", default="anf", help="a = plain, n = NIS only, f = NIS + innovations")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are measured (default: this one)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("innov_stream_rate: needs a GPU")
    import numpy as np
    import yaml
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    forms = [f for f in "anf" if f in args.forms]
    record = {"tool": "tools/innov_stream_rate.py", "device": torch.cuda.get_device_name(0), "root": os.path.relpath(root, ROOT),
              "bytes_per_target_tick": {f: BYTES[f] for f in forms},
              "expected_time_ratio_if_hbm_bound": {f: BYTES[f] / STATE_B for f in forms if f != "a"},
              "note": "algorithmic bytes: 872 B/target/tick of state (read + write) and measurements, + 8 B/target/tick of NIS in (n) "
                      "and (f), + 48 B/target/tick of innovations (6 doubles) in (f).  HBM-side bytes (PMC) were not collected.",
              "configs": {}}
    for cfg in args.configs.split(","):
        parts = CONFIGS[cfg]
        models = {}
        for n, _ in parts:   # Q, R, P of the shipped model file (row-major flow sequences)
            with open(os.path.join(root, "models", "model_%s_params.yaml" % n)) as f:
                node = yaml.safe_load(f)
            ns, nm = te.MODEL_DIMS[te.MODEL_TYPES[n]]
            models[n] = dict(Q=np.array(node["Q"], dtype=np.float64).reshape(ns, ns), R=np.array(node["R"], dtype=np.float64).reshape(nm, nm),
                             P=np.array(node["P"], dtype=np.float64).reshape(ns, ns))
        mgr = te.TargetManager(dtype="f64")
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        meas, base = [], 0
        for k, (name, n) in enumerate(parts):
            m = models[name]
            st = make_stream(te.MODEL_TYPES[name], n, RING, DT, SEED + 17 * k, dtype="f64")
            ids = np.arange(n, dtype=np.uint32) + base
            base += n
            mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"])
            meas.append(st["meas"])
        bs = mgr.batches()
        ntot = sum(b.size for b in bs)
        assert mgr.population_tick()
        nis = [torch.empty((1, b.size), dtype=torch.float64, device="cuda") for b in bs]
        nu = [torch.empty((1, b.meas_dim, b.size), dtype=torch.float64, device="cuda") for b in bs]

        def run(form, ticks):
            if form == "a":
                mgr.step_sequence_all(DT, meas, use_graph=0, n_ticks=ticks)
            elif form == "n":
                mgr.step_sequence_all(DT, meas, use_graph=0, n_ticks=ticks, innov=[(s, None) for s in nis])
            else:
                mgr.step_sequence_all(DT, meas, use_graph=0, n_ticks=ticks, innov=list(zip(nis, nu)))

        def timed(form, ticks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            run(form, ticks)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0

        for f in forms:   # warm-up (and the first-use allocations, e.g. the second record buffers of A -> B ticks)
            run(f, 4 * RING)
        est, _ = timed(forms[0], 2 * RING)
        ticks = max(RING, int(args.seconds / (est / (2 * RING))) // RING * RING)
        res = {f: [] for f in forms}
        for rep in range(args.reps):
            for f in (forms if rep % 2 == 0 else forms[::-1]):
                gpu_s, wall_s = timed(f, ticks)
                res[f].append(dict(tick_us=gpu_s / ticks * 1e6, wall_tick_us=wall_s / ticks * 1e6))
        out = {"targets": ntot, "ticks_per_rep": ticks, "shared_axes": [int(b.shared_axes) for b in bs], "forms": {}}
        for f in forms:
            t = [r["tick_us"] for r in res[f]]
            med = statistics.median(t)
            out["forms"][f] = dict(reps=res[f], tick_us_median=med, tick_us_min=min(t), tick_us_max=max(t), spread=(max(t) - min(t)) / med,
                                   gbps=BYTES[f] * ntot / (med * 1e-6) / 1e9, frac_of_8TBs=BYTES[f] * ntot / (med * 1e-6) / PEAK)
        for f in forms:
            if f != "a" and "a" in forms:
                out["%s_over_a_time" % f] = out["forms"][f]["tick_us_median"] / out["forms"]["a"]["tick_us_median"]
                out["%s_over_a_bytes" % f] = BYTES[f] / STATE_B
        record["configs"][cfg] = out
        print(cfg, json.dumps({f: (round(v["tick_us_median"], 1), round(v["frac_of_8TBs"], 3), round(v["spread"], 4))
                                for f, v in out["forms"].items()}), flush=True)
        mgr.close()
        del meas, nis, nu
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
