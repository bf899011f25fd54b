#!/usr/bin/env python3
"""The cost of the re-acquisition inside the gated ticks at the large mixed configurations (GPU only).  For cfg4_1gpu (500 000
angular-rates + 500 000 angular-velocities, fp64, the shared-axes form) and cfg4_4m (2 000 000 + 2 000 000) -- the sizes of
profiles/r11_gate_stream.json -- it times three forms of the node's loop, eager target_manager_step_sequence_all ticks over a
measurement ring of 16 ticks:
  (g) gated      the population tick with a NIS-only stream and the gate nis_max = 300 on every batch, clean ring: the parent's tick
  (r) reacquire  the same with the policy K = 3 and one event row per batch (target_manager_step_sequence_all_reacquire)
  (j) jump       the same on a second ring in which 1 target in 8 is seen +0.5 m away on ring entries 8..15: it is rejected twice and
                 re-initialised on the third tick of each half of the ring
HIP events around each timed region, a warm-up per form, forms alternated and repeated (--reps): the record has every
repetition, the median and the spread.  By bytes the policy adds about 11 B per target and tick -- NIS row read (8), run read
and written (2), event byte (1) -- to the gated tick's 888, plus one small launch per batch and tick.
--forms g --root <tree> times the gated tick of another checkout of the project (its package and built library) with this same
tool; --versus <tree> does the whole comparison: fresh processes of this checkout (g, r) and of that one (g) alternated --rounds
times, then one process of this checkout with all three forms -- the ring with the jump leaves the tiles non-uniform for every
form after it in its process, so its three figures are compared with each other only.  All records go into one file.
  python tools/reacquire_rate.py --versus <parent checkout> --out profiles/r12_reacquire.json [--seconds 0.5] [--reps 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"cfg4_1gpu": [("angular_rates", 500_000), ("angular_velocities", 500_000)],
           "cfg4_4m": [("angular_rates", 2_000_000), ("angular_velocities", 2_000_000)]}
GATED_B, POLICY_B, PEAK = 888, 11, 8.0e12
BYTES = {"g": GATED_B, "r": GATED_B + POLICY_B, "j": GATED_B + POLICY_B}
GAMMA, K = 300.0, 3
RING, DT, SEED = 16, 0.004, 20240004


def versus(args):
    """fresh processes of this checkout (g, r, j) and of args.versus (g) alternated; one record"""
    record = {"tool": "tools/reacquire_rate.py --versus", "rounds": [],
              "note": "every entry is a fresh process; 'this' (g, r on the clean ring) and 'parent' (g) alternate; 'this_jump' runs g, r, j in one "
                      "process, all three on tiles the jump has left non-uniform"}
    for rnd in range(args.rounds):
        for who, root, forms in (("this", ROOT, "gr"), ("parent", os.path.abspath(args.versus), "g")) + ((("this_jump", ROOT, "grj"),) if rnd == args.rounds - 1 else ()):
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--root", root, "--forms", forms, "--out", tmp.name, "--seconds",
                                       str(args.seconds), "--reps", str(args.reps), "--configs", args.configs], timeout=args.child_timeout)
                record["rounds"].append({"round": rnd, "who": who, "record": json.load(open(tmp.name))})
    summary = {}
    for cfg in args.configs.split(","):
        med = {}
        for key, who, form in (("parent_g", "parent", "g"), ("this_g", "this", "g"), ("this_r", "this", "r"), ("jump_g", "this_jump", "g"),
                               ("jump_r", "this_jump", "r"), ("jump_j", "this_jump", "j")):
            v = [r["record"]["configs"][cfg]["forms"][form] for r in record["rounds"] if r["who"] == who]
            med[key] = dict(tick_us_median_of_processes=statistics.median(x["tick_us_median"] for x in v),
                            tick_us_per_process=[x["tick_us_median"] for x in v], largest_spread=max(x["spread"] for x in v))
        spread = max(m["largest_spread"] for m in med.values())
        base = med["parent_g"]["tick_us_median_of_processes"]
        summary[cfg] = dict(med, largest_spread_reported=spread,
                            this_g_over_parent_g=med["this_g"]["tick_us_median_of_processes"] / base,
                            agree_within_3_spreads=abs(med["this_g"]["tick_us_median_of_processes"] / base - 1.0) <= 3.0 * spread,
                            this_r_over_parent_g=med["this_r"]["tick_us_median_of_processes"] / base,
                            jump_process_r_over_g=med["jump_r"]["tick_us_median_of_processes"] / med["jump_g"]["tick_us_median_of_processes"],
                            jump_process_j_over_g=med["jump_j"]["tick_us_median_of_processes"] / med["jump_g"]["tick_us_median_of_processes"],
                            r_minus_parent_g_us=med["this_r"]["tick_us_median_of_processes"] - base,
                            expected_ratio_by_bytes=(GATED_B + POLICY_B) / GATED_B)
        print(cfg, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in summary[cfg].items() if not isinstance(v, dict)}), flush=True)
    record["summary"] = summary
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="cfg4_1gpu,cfg4_4m")
    ap.add_argument("--forms", default="grj", help="g = gated (clean ring), r = gated with K = 3 and an event row, j = the same on the ring with the jump")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are measured (default: this one)")
    ap.add_argument("--versus", default=None, help="another checkout (the parent commit, built): alternate fresh processes of both")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=280.0)
    args = ap.parse_args()
    if args.versus:
        return versus(args)
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reacquire_rate: needs a GPU")
    import numpy as np
    import yaml
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    forms = [f for f in "grj" if f in args.forms]
    record = {"tool": "tools/reacquire_rate.py", "nis_max": GAMMA, "max_rejects": K, "device": torch.cuda.get_device_name(0),
              "root": os.path.relpath(root, ROOT), "bytes_per_target_tick": {f: BYTES[f] for f in forms},
              "note": "algorithmic bytes: 888 B/target/tick of the gated tick (state, measurements, NIS, counter) + 11 B/target/tick of the "
                      "policy's streaming pass in (r) and (j).  HBM-side bytes (PMC) were not collected.",
              "configs": {}}
    for cfg in args.configs.split(","):
        parts = CONFIGS[cfg]
        models = {}
        for n, _ in parts:
            with open(os.path.join(root, "models", "model_%s_params.yaml" % n)) as f:
                node = yaml.safe_load(f)
            ns, nm = te.MODEL_DIMS[te.MODEL_TYPES[n]]
            models[n] = dict(Q=np.array(node["Q"], dtype=np.float64).reshape(ns, ns), R=np.array(node["R"], dtype=np.float64).reshape(nm, nm),
                             P=np.array(node["P"], dtype=np.float64).reshape(ns, ns))
        mgr = te.TargetManager(dtype="f64")
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        meas, jump, base = [], [], 0
        for k, (name, n) in enumerate(parts):
            m = models[name]
            st = make_stream(te.MODEL_TYPES[name], n, RING, DT, SEED + 17 * k, dtype="f64")
            ids = np.arange(n, dtype=np.uint32) + base
            base += n
            mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"])
            meas.append(st["meas"])
            if "j" in forms:
                d = st["meas"].clone()
                d[RING // 2:, 0, 0:n:8] += 0.5
                jump.append(d)
        bs = mgr.batches()
        ntot = sum(b.size for b in bs)
        assert mgr.population_tick()
        nis = [torch.empty((1, b.size), dtype=torch.float64, device="cuda") for b in bs]
        events = [torch.zeros((1, b.size), dtype=torch.uint8, device="cuda") for b in bs]

        def run(form, ticks):
            kw = dict(use_graph=0, n_ticks=ticks, innov=[(s, None) for s in nis], gate=GAMMA)
            if form == "g":
                mgr.step_sequence_all(DT, meas, **kw)
            else:
                mgr.step_sequence_all(DT, jump if form == "j" else meas, reacquire=[(K, e) for e in events], **kw)

        def timed(form, ticks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            run(form, ticks)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0

        for f in forms:
            run(f, 4 * RING)
        est, _ = timed(forms[0], 2 * RING)
        ticks = max(RING, int(args.seconds / (est / (2 * RING))) // RING * RING)
        res = {f: [] for f in forms}
        for rep in range(args.reps):
            for f in (forms if rep % 2 == 0 else forms[::-1]):
                gpu_s, wall_s = timed(f, ticks)
                res[f].append(dict(tick_us=gpu_s / ticks * 1e6, wall_tick_us=wall_s / ticks * 1e6))
        out = {"targets": ntot, "ticks_per_rep": ticks, "shared_axes": [int(b.shared_axes) for b in bs], "forms": {}}
        if "j" in forms:   # what one pass over the ring with the jump does: re-initialisations per target and tick
            ev = [torch.zeros((RING, b.size), dtype=torch.uint8, device="cuda") for b in bs]
            mgr.step_sequence_all(DT, jump, use_graph=0, n_ticks=RING, innov=[(s, None) for s in nis], gate=GAMMA, reacquire=[(K, e) for e in ev])
            torch.cuda.synchronize()
            out["reinitialised_share_j"] = float(sum(int((e >= 128).sum()) for e in ev)) / (ntot * RING)
        for f in forms:
            t = [r["tick_us"] for r in res[f]]
            med = statistics.median(t)
            out["forms"][f] = dict(reps=res[f], tick_us_median=med, tick_us_min=min(t), tick_us_max=max(t), spread=(max(t) - min(t)) / med,
                                   gbps=BYTES[f] * ntot / (med * 1e-6) / 1e9, frac_of_8TBs=BYTES[f] * ntot / (med * 1e-6) / PEAK)
        for f in forms:
            if f != "g" and "g" in forms:
                out["%s_over_g_time" % f] = out["forms"][f]["tick_us_median"] / out["forms"]["g"]["tick_us_median"]
                out["%s_over_g_bytes" % f] = BYTES[f] / BYTES["g"]
        record["configs"][cfg] = out
        print(cfg, json.dumps({f: (round(v["tick_us_median"], 1), round(v["frac_of_8TBs"], 3), round(v["spread"], 4))
                                for f, v in out["forms"].items()}), flush=True)
        mgr.close()
        del meas, nis, jump, events
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
