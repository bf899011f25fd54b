#!/usr/bin/env python3
"""A temporally fused replay of a whole manager: one launch (step_fused_all) against the per-batch fused calls in batch order on
one manager, which is how the same work is done without the manager-level call (GPU only).  Shapes:
  a4x2500        four models x 2 500 targets, fp64, 100 ticks per call
  a4x2500_dt     the same with a time-step schedule (jittered dt, one 0.0 entry)
  cfg3_1m        500 000 angular-rates + 500 000 angular-velocities targets, fp64 (BASELINE configs[3]), 20 ticks per call
each plain (no stream) and gated (NIS-only stream on every batch, nis_max = 300, K = 3 with event rows).  Forms:
  (m) manager    ONE TargetManager.step_fused_all call per replay
  (b) per batch  Batch.step_fused(...) per batch, in batch order, on the manager's stream
HIP events around each timed region (a region = as many calls as fill --seconds), a warm-up per shape, --reps repetitions per
process; the two forms run in FRESH PROCESSES that alternate (--rounds of m, b).  The record keeps every repetition, the median per
process and the spread ((max - min) / median over a process's repetitions); a shape's verdict is the ratio of the medians over the
processes against a margin of three times the largest spread reported for that shape.  All figures are EFFECTIVE times per tick --
the state stays in registers over a call's ticks -- and are not throughput values; HBM-side bytes (PMC) are not collected.
  python tools/fused_all_rate.py --out profiles/fused_all_rate.json [--seconds 0.2] [--reps 3] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = [("angular_rates", 2500), ("angular_velocities", 2500), ("uniform_acceleration", 2500), ("uniform_velocity", 2500)]
SHAPES = {"a4x2500": (FOUR, 100, False), "a4x2500_dt": (FOUR, 100, True),
          "cfg3_1m": ([("angular_rates", 500_000), ("angular_velocities", 500_000)], 20, False)}
GAMMA, K, DT, SEED = 300.0, 3, 0.004, 20240021
NAMES = {"m": "manager call (one launch)", "b": "per-batch fused calls"}


def drive(args):
    record = {"tool": "tools/fused_all_rate.py", "rounds": [],
              "note": "every entry is a fresh process; the forms m and b alternate.  Effective figures (temporal fusion: the state stays in "
                      "registers over a call's ticks).  PMC bytes were not collected."}
    for rnd in range(args.rounds):
        for form in ("mb" if rnd % 2 == 0 else "bm"):
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--form", form, "--out", tmp.name, "--seconds", str(args.seconds),
                                       "--reps", str(args.reps), "--shapes", args.shapes], timeout=args.child_timeout)
                record["rounds"].append({"round": rnd, "form": form, "record": json.load(open(tmp.name))})
    summary = {}
    for shape in args.shapes.split(","):
        for mode in ("plain", "gated"):
            key = "%s_%s" % (shape, mode)
            per = {f: [r["record"]["shapes"][key] for r in record["rounds"] if r["form"] == f] for f in "mb"}
            med = {f: statistics.median(x["tick_us_median"] for x in per[f]) for f in "mb"}
            spread = max(x["spread"] for f in "mb" for x in per[f])
            ratio = med["m"] / med["b"]
            summary[key] = dict(manager_tick_us=med["m"], per_batch_tick_us=med["b"], manager_over_per_batch=ratio,
                                per_process={f: [x["tick_us_median"] for x in per[f]] for f in "mb"}, largest_spread_reported=spread,
                                margin=3.0 * spread, manager_no_slower_within_margin=ratio <= 1.0 + 3.0 * spread,
                                served_one_launch=all(x["served"] == 1 for x in per["m"]))
            print(key, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in summary[key].items() if not isinstance(v, dict)}), flush=True)
    record["summary"] = summary
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--form", default=None, help="m or b: measure that form in this process (the driver starts these)")
    ap.add_argument("--child-timeout", type=float, default=280.0)
    args = ap.parse_args()
    if args.reps < 3 or args.rounds < 1:
        raise SystemExit("fused_all_rate: at least 3 repetitions")
    if args.form is None:
        return drive(args)
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fused_all_rate: needs a GPU")
    import numpy as np
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    import yaml
    form = args.form

    def model_params(name):   # Q, R, P0 of a shipped model file (row-major)
        with open(os.path.join(ROOT, "models", "model_%s_params.yaml" % name)) as f:
            node = yaml.safe_load(f)
        n, m = te.MODEL_DIMS[te.MODEL_TYPES[name]]
        return dict(Q=np.array(node["Q"]).reshape(n, n), R=np.array(node["R"]).reshape(m, m), P=np.array(node["P"]).reshape(n, n))
    record = {"tool": "tools/fused_all_rate.py", "form": form, "form_name": NAMES[form], "nis_max": GAMMA, "max_rejects": K,
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    for shape in args.shapes.split(","):
        parts, ticks, scheduled = SHAPES[shape]
        dt = DT
        if scheduled:
            jit = np.random.default_rng(SEED).uniform(0.6, 1.6, ticks)
            jit[ticks // 3] = 0.0
            dt = list(DT * jit)
        mgr = te.TargetManager(dtype="f64", lanes_per_target=301, shared_axes=False)
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        meas, base = [], 0
        for k, (name, n) in enumerate(parts):
            mdl = model_params(name)
            st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, SEED + 17 * k, dtype="f64")
            ids = np.arange(n, dtype=np.uint32) + base
            base += n
            assert mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=mdl["Q"], R=mdl["R"], P0=mdl["P"]) == n
            meas.append(st["meas"])
        bs = mgr.batches()
        assert len(bs) == len(parts)
        nis = [(torch.empty((ticks, b.size), dtype=torch.float64, device="cuda"), None) for b in bs]
        events = [(K, torch.zeros((ticks, b.size), dtype=torch.uint8, device="cuda")) for b in bs]
        for mode in ("plain", "gated"):
            kw = dict(innov=nis, gate=GAMMA, reacquire=events) if mode == "gated" else {}

            def call():
                if form == "m":
                    mgr.step_fused_all(dt, meas, **kw)
                else:
                    for i, b in enumerate(bs):
                        if mode == "gated":
                            b.step_fused(dt, meas[i], innov=nis[i], gate=GAMMA, reacquire=events[i])
                        else:
                            b.step_fused(dt, meas[i])

            def timed(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e-3
            for _ in range(3):
                call()
            calls = max(3, int(args.seconds / (timed(3) / 3)))
            reps = [dict(tick_us=timed(calls) / (calls * ticks) * 1e6, calls=calls) for _ in range(args.reps)]
            t = [r["tick_us"] for r in reps]
            med = statistics.median(t)
            out = dict(parts=parts, ticks_per_call=ticks, scheduled=scheduled, mode=mode, reps=reps, tick_us_median=med, tick_us_min=min(t),
                       tick_us_max=max(t), spread=(max(t) - min(t)) / med, effective=True,
                       served=int(mgr.fused_all_served(gated=mode == "gated", scheduled=scheduled)))
            if mode == "gated":
                torch.cuda.synchronize()
                out["rejected_share_last_call"] = float(sum((x[0] > GAMMA).sum().item() for x in nis)) / sum(x[0].numel() for x in nis)
            record["shapes"]["%s_%s" % (shape, mode)] = out
            print(shape, mode, NAMES[form], round(med, 3), "us per tick, spread", round(out["spread"], 4), flush=True)
        mgr.close()
        del meas, nis, events
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
