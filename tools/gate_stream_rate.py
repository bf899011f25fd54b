#!/usr/bin/env python3
"""The NIS validation gate at the large mixed configurations (GPU only).  For cfg4_1gpu (500 000 angular-rates + 500 000
angular-velocities, fp64) and cfg4_4m (2 000 000 + 2 000 000) -- the sizes of profiles/r09_innov_stream.json -- it times four forms
of the node's loop, eager target_manager_step_sequence_all ticks over a measurement ring:
  (a) plain   the population tick alone
  (n) nis     the population tick with a NIS-only stream per batch (target_manager_step_sequence_all_innov, one row overwritten)
  (g) gated   the same with the gate nis_max = 300 on every batch (target_manager_step_sequence_all_gated) on the clean ring
  (o) gated   the same on a second ring with +0.5 m on a Bernoulli(1/12) subset of the measurements: rejections split the tiles
              that the clean stream leaves uniform
HIP events around each timed region, a warm-up per form, forms alternated and repeated (--reps): the record has every
repetition, the median and the spread.  By bytes the gate adds 8 B per target and tick to the NIS-only tick -- the read-modify-
write of the per-target measurement counter -- and beyond that whatever occupancy its kernels lose.
--forms an --root <tree> times the plain and the NIS-only tick of another checkout of the project (its package and built
library) with this same tool: the comparison against the parent commit.
  python tools/gate_stream_rate.py --out profiles/r11_gate_stream.json [--seconds 1.0] [--reps 3] [--configs cfg4_1gpu,cfg4_4m]
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
STATE_B, NIS_B, COUNT_B, PEAK = 872, 8, 8, 8.0e12
BYTES = {"a": STATE_B, "n": STATE_B + NIS_B, "g": STATE_B + NIS_B + COUNT_B, "o": STATE_B + NIS_B + COUNT_B}
GAMMA = 300.0
RING, DT, SEED = 16, 0.004, 20240004


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="cfg4_1gpu,cfg4_4m")
    ap.add_argument("--forms", default="ango", help="a = plain, n = NIS only, g = gated NIS only (clean ring), o = gated, ring with outliers")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are measured (default: this one)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gate_stream_rate: needs a GPU")
    import numpy as np
    import yaml
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    forms = [f for f in "ango" if f in args.forms]
    record = {"tool": "tools/gate_stream_rate.py", "nis_max": GAMMA, "device": torch.cuda.get_device_name(0), "root": os.path.relpath(root, ROOT),
              "bytes_per_target_tick": {f: BYTES[f] for f in forms},
              "expected_time_ratio_if_hbm_bound": {f: BYTES[f] / STATE_B for f in forms if f != "a"},
              "note": "algorithmic bytes: 872 B/target/tick of state (read + write) and measurements, + 8 B/target/tick of NIS in (n), (g) "
                      "and (o), + 8 B/target/tick for the measurement counter's read-modify-write in (g) and (o).  (o): a second ring with "
                      "+0.5 m on a Bernoulli(1/12) subset of the measurements.  HBM-side bytes (PMC) were not collected.",
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
        meas, dirty, base = [], [], 0
        for k, (name, n) in enumerate(parts):
            m = models[name]
            st = make_stream(te.MODEL_TYPES[name], n, RING, DT, SEED + 17 * k, dtype="f64")
            ids = np.arange(n, dtype=np.uint32) + base
            base += n
            mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"])
            meas.append(st["meas"])
            if "o" in forms:   # the same ring with the outliers
                rng = np.random.default_rng(5 + k)
                d = st["meas"].clone()
                hit = torch.from_numpy(rng.random((RING, n)) < 1.0 / 12.0).cuda()
                axis = torch.from_numpy(rng.integers(0, 3, (RING, n))).cuda()
                for c in range(3):
                    d[:, c, :n] += 0.5 * (hit & (axis == c)).to(d.dtype)
                dirty.append(d)
        bs = mgr.batches()
        ntot = sum(b.size for b in bs)
        assert mgr.population_tick()
        nis = [torch.empty((1, b.size), dtype=torch.float64, device="cuda") for b in bs]

        def run(form, ticks):
            if form == "a":
                mgr.step_sequence_all(DT, meas, use_graph=0, n_ticks=ticks)
            elif form == "n":
                mgr.step_sequence_all(DT, meas, use_graph=0, n_ticks=ticks, innov=[(s, None) for s in nis])
            else:
                mgr.step_sequence_all(DT, dirty if form == "o" else meas, use_graph=0, n_ticks=ticks, innov=[(s, None) for s in nis], gate=GAMMA)

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
        if "o" in forms:   # what the gate does to the two rings: the rejected share of one more tick of each
            for key, ring in (("g", meas), ("o", dirty)):
                if key in forms:
                    mgr.step_sequence_all(DT, ring, use_graph=0, n_ticks=1, innov=[(s, None) for s in nis], gate=GAMMA)
                    torch.cuda.synchronize()
                    out["rejected_share_%s" % key] = float(sum(int((s > GAMMA).sum()) for s in nis)) / ntot
        for f in forms:
            t = [r["tick_us"] for r in res[f]]
            med = statistics.median(t)
            out["forms"][f] = dict(reps=res[f], tick_us_median=med, tick_us_min=min(t), tick_us_max=max(t), spread=(max(t) - min(t)) / med,
                                   gbps=BYTES[f] * ntot / (med * 1e-6) / 1e9, frac_of_8TBs=BYTES[f] * ntot / (med * 1e-6) / PEAK)
        for f in forms:
            for base_form in ("a", "n"):
                if f != base_form and base_form in forms and f != "a":
                    out["%s_over_%s_time" % (f, base_form)] = out["forms"][f]["tick_us_median"] / out["forms"][base_form]["tick_us_median"]
                    out["%s_over_%s_bytes" % (f, base_form)] = BYTES[f] / BYTES[base_form]
        record["configs"][cfg] = out
        print(cfg, json.dumps({f: (round(v["tick_us_median"], 1), round(v["frac_of_8TBs"], 3), round(v["spread"], 4))
                                for f, v in out["forms"].items()}), flush=True)
        mgr.close()
        del meas, nis, dirty
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
