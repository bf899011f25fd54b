#!/usr/bin/env python3
"""The effective time per tick of a fused gated call (GPU only).  For 10^4 uniform-velocity fp64 targets (BASELINE.json configs[1])
and 10^6 angular-rates fp64 targets it times 20-tick calls over a clean measurement ring of 20 ticks, NIS-only stream, the gate
nis_max = 300, the policy K = 3 with event rows:
  (f) fused gate   ONE step_fused(..., innov=, gate=, reacquire=) call: one launch for the 20 ticks (this checkout only)
  (e) eager        step_sequence(..., innov=, gate=, reacquire=), use_graph 0: the gated tick and the policy launch per tick
  (g) graph        the same sequence as a recorded graph, replayed
  (p) plain fused  step_fused without stream, gate or policy: the path this feature leaves unchanged
HIP events around each timed region (a region = as many 20-tick calls as fill --seconds), a warm-up per form, forms alternated and
repeated (--reps): the record has every repetition, the median and the spread.  The figures of (f) and (p) are EFFECTIVE ones --
the state stays in registers over the 20 ticks, so they are not comparable with a tick that moves its state -- and are reported
as such, never as a throughput value.  HBM-side bytes (PMC) are not collected.
--forms egp --root <tree> times another checkout of the project (its package and built library) with this same tool; --versus
<tree> does the whole comparison: fresh processes of this checkout (f, e, g, p) and of that one (e, g, p) alternated --rounds
times.  All records go into one file.
  python tools/fused_gate_rate.py --versus <parent checkout> --out profiles/fused_gate_rate.json [--seconds 0.3] [--reps 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"uv_1e4": ("uniform_velocity", 10_000), "ar_1e6": ("angular_rates", 1_000_000)}
GAMMA, K, TICKS, DT, SEED = 300.0, 3, 20, 0.004, 20240013
NAMES = {"f": "fused gate", "e": "eager sequence", "g": "recorded graph", "p": "plain fused"}


def versus(args):
    record = {"tool": "tools/fused_gate_rate.py --versus", "rounds": [],
              "note": "every entry is a fresh process; 'this' (f, e, g, p) and 'parent' (e, g, p) alternate.  f and p are effective figures "
                      "(temporal fusion: the state stays in registers over the call's 20 ticks).  PMC bytes were not collected."}
    for rnd in range(args.rounds):
        for who, root, forms in (("this", ROOT, "fegp"), ("parent", os.path.abspath(args.versus), "egp")):
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--root", root, "--forms", forms, "--out", tmp.name, "--seconds",
                                       str(args.seconds), "--reps", str(args.reps), "--configs", args.configs], timeout=args.child_timeout)
                rec = json.load(open(tmp.name))
                rec["root"] = who
                record["rounds"].append({"round": rnd, "who": who, "record": rec})
    summary = {}
    for cfg in args.configs.split(","):
        med = {}
        for who, forms in (("this", "fegp"), ("parent", "egp")):
            for f in forms:
                v = [r["record"]["configs"][cfg]["forms"][f] for r in record["rounds"] if r["who"] == who]
                med["%s_%s" % (who, f)] = dict(tick_us_median_of_processes=statistics.median(x["tick_us_median"] for x in v),
                                               tick_us_per_process=[x["tick_us_median"] for x in v], largest_spread=max(x["spread"] for x in v))
        spread = max(m["largest_spread"] for m in med.values())
        t = {k: m["tick_us_median_of_processes"] for k, m in med.items()}
        summary[cfg] = dict(med, largest_spread_reported=spread,
                            effective_fused_gate_over_parent_eager=t["this_f"] / t["parent_e"],
                            effective_fused_gate_over_parent_graph=t["this_f"] / t["parent_g"],
                            fused_gate_faster_than_parent_graph=t["this_f"] < t["parent_g"],
                            effective_fused_gate_over_plain_fused=t["this_f"] / t["this_p"],
                            plain_fused_this_over_parent=t["this_p"] / t["parent_p"],
                            plain_fused_agrees_within_3_spreads=abs(t["this_p"] / t["parent_p"] - 1.0) <= 3.0 * spread)
        print(cfg, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in summary[cfg].items() if not isinstance(v, dict)}), flush=True)
    record["summary"] = summary
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="uv_1e4,ar_1e6")
    ap.add_argument("--forms", default="fegp", help="f = fused gate, e = eager gated sequence, g = the sequence as a recorded graph, p = plain step_fused")
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
        raise SystemExit("fused_gate_rate: needs a GPU")
    import numpy as np
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    forms = [f for f in "fegp" if f in args.forms]
    record = {"tool": "tools/fused_gate_rate.py", "nis_max": GAMMA, "max_rejects": K, "ticks_per_call": TICKS, "device": torch.cuda.get_device_name(0),
              "forms": {f: NAMES[f] for f in forms}, "configs": {}}
    for cfg in args.configs.split(","):
        name, n = CONFIGS[cfg]
        st = make_stream(te.MODEL_TYPES[name], n, TICKS, DT, SEED, dtype="f64")
        meas = st["meas"]
        p0 = st["p0"].cpu().numpy()
        res = {f: [] for f in forms}
        out = {"model": name, "targets": n, "forms": {}}
        mgrs = {}
        for f in forms:   # a manager per form: every form steps a batch with the same history
            mgr = te.TargetManager(os.path.join(root, "models", "model_%s_params.yaml" % name), dtype="f64")
            mgr.set_stream(torch.cuda.current_stream().cuda_stream)
            mgr.init_batch(np.arange(n, dtype=np.uint32), DT, 0.0, p0)
            mgrs[f] = (mgr, mgr.batches()[0])
        nis = torch.empty((TICKS, n), dtype=torch.float64, device="cuda")
        events = torch.zeros((TICKS, n), dtype=torch.uint8, device="cuda")

        def call(f):
            b = mgrs[f][1]
            if f == "f":
                b.step_fused(DT, meas, innov=(nis, None), gate=GAMMA, reacquire=(K, events))
            elif f == "p":
                b.step_fused(DT, meas)
            else:
                b.step_sequence(DT, meas, use_graph=(f == "g"), innov=(nis, None), gate=GAMMA, reacquire=(K, events))

        def timed(f, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                call(f)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        calls = {}
        for f in forms:
            for _ in range(3):
                call(f)
            est = timed(f, 3) / 3
            calls[f] = max(3, int(args.seconds / est))
        if "f" in forms:
            out["fused_gate_served"] = int(mgrs["f"][1].fused_gate_served)
        for rep in range(args.reps):
            for f in (forms if rep % 2 == 0 else forms[::-1]):
                res[f].append(dict(tick_us=timed(f, calls[f]) / (calls[f] * TICKS) * 1e6, calls=calls[f]))
        torch.cuda.synchronize()
        out["rejected_share_last_call"] = float((nis > GAMMA).sum().item()) / nis.numel() if ("f" in forms or "e" in forms or "g" in forms) else None
        for f in forms:
            t = [r["tick_us"] for r in res[f]]
            med = statistics.median(t)
            out["forms"][f] = dict(reps=res[f], tick_us_median=med, tick_us_min=min(t), tick_us_max=max(t), spread=(max(t) - min(t)) / med,
                                   effective=f in "fp")
        record["configs"][cfg] = out
        print(cfg, json.dumps({NAMES[f]: (round(v["tick_us_median"], 2), round(v["spread"], 4)) for f, v in out["forms"].items()}), flush=True)
        for mgr, _ in mgrs.values():
            mgr.close()
        del meas, nis, events, st
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
