#!/usr/bin/env python3
"""The time per tick of the calls with a time step per tick (GPU only).  For 10^4 uniform-velocity fp64 targets (BASELINE.json
configs[1]) and 10^6 angular-rates fp64 targets it times 20-tick calls over a clean measurement ring of 20 ticks with a jittered
schedule dt[s] = DT * f[s], f seeded over [0.25, 2]:
  (d) fused schedule        ONE step_fused(dt=schedule) call: one launch for the 20 ticks, tick s reads dt[s] from the device table
  (D) fused gated schedule  ONE step_fused(dt=schedule, innov=, gate=, reacquire=) call (NIS-only stream, nis_max 300, K = 3, event rows)
  (s) eager schedule        step_sequence(dt=schedule), use_graph 0: a launch per tick, its dt passed by value
  (r) recorded schedule     the same sequence as a recorded graph, replayed (the same schedule every call: one recording)
  (p) plain fused           step_fused with a scalar dt: the path this feature leaves unchanged
  (f) fused gate            step_fused(..., innov=, gate=, reacquire=) with a scalar dt: likewise unchanged
HIP events around each timed region (a region = as many 20-tick calls as fill --seconds), a warm-up per form, forms alternated and
repeated (--reps): the record has every repetition, the median and the spread.  The figures of d, D, p and f are EFFECTIVE ones --
the state stays in registers over the 20 ticks, so they are not comparable with a tick that moves its state -- and are reported
as such, never as a throughput value.  HBM-side bytes (PMC) are not collected.
--forms pf --root <tree> times another checkout of the project (its package and built library) with this same tool; --versus
<tree> does the whole comparison: fresh processes of this checkout (all forms) and of that one (p, f) alternated --rounds times,
and with --bench-steps K the headline line of each checkout's bench.py (--gpus 1 --steps K --warmup W) alternated likewise.
All records go into one file.  The summary holds the unchanged paths (p, f, the bench line) to three times the largest spread of
the record, and the new fused forms over the parent's scalar fused call to 1 plus three times the spread of the two forms of
that ratio; --summarise-from <record> recomputes it from a record's rounds (no GPU).
  python tools/dt_schedule_rate.py --versus <parent checkout> --out profiles/dt_schedule_rate.json [--seconds 0.3] [--reps 3]
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
NAMES = {"d": "fused schedule", "D": "fused gated schedule", "s": "eager schedule sequence", "r": "recorded schedule sequence",
         "p": "plain fused (scalar dt)", "f": "fused gate (scalar dt)"}
ALL, OLD = "dDsrpf", "pf"
EFFECTIVE = "dDpf"


def summarise(record, configs):
    """the medians over the processes and the ratios, from the rounds of a --versus record (no GPU needed: --summarise-from)"""
    summary = {}
    for cfg in configs:
        med = {}
        for who, forms in (("this", ALL), ("parent", OLD)):
            for f in forms:
                v = [r["record"]["configs"][cfg]["forms"][f] for r in record["rounds"] if r["who"] == who]
                med["%s_%s" % (who, f)] = dict(tick_us_median_of_processes=statistics.median(x["tick_us_median"] for x in v),
                                               tick_us_per_process=[x["tick_us_median"] for x in v], largest_spread=max(x["spread"] for x in v))
        spread = max(m["largest_spread"] for m in med.values())
        t = {k: m["tick_us_median_of_processes"] for k, m in med.items()}

        def own(*keys):   # the largest spread among the forms of one ratio
            return max(med[k]["largest_spread"] for k in keys)
        summary[cfg] = dict(med, largest_spread_reported=spread,
                            plain_fused_this_over_parent=t["this_p"] / t["parent_p"],
                            plain_fused_agrees_within_3_spreads=abs(t["this_p"] / t["parent_p"] - 1.0) <= 3.0 * spread,
                            fused_gate_this_over_parent=t["this_f"] / t["parent_f"],
                            fused_gate_agrees_within_3_spreads=abs(t["this_f"] / t["parent_f"] - 1.0) <= 3.0 * spread,
                            effective_fused_schedule_over_parent_plain_fused=t["this_d"] / t["parent_p"],
                            fused_schedule_spread_of_its_two_forms=own("this_d", "parent_p"),
                            fused_schedule_within_1_plus_3_spreads_of_its_two_forms=t["this_d"] / t["parent_p"] <= 1.0 + 3.0 * own("this_d", "parent_p"),
                            fused_schedule_extra_us_per_20_tick_call=(t["this_d"] - t["parent_p"]) * TICKS,
                            effective_fused_gated_schedule_over_parent_fused_gate=t["this_D"] / t["parent_f"],
                            fused_gated_schedule_spread_of_its_two_forms=own("this_D", "parent_f"),
                            fused_gated_schedule_within_1_plus_3_spreads_of_its_two_forms=t["this_D"] / t["parent_f"] <= 1.0 + 3.0 * own("this_D", "parent_f"),
                            fused_gated_schedule_extra_us_per_20_tick_call=(t["this_D"] - t["parent_f"]) * TICKS,
                            effective_fused_schedule_over_eager_schedule=t["this_d"] / t["this_s"],
                            effective_fused_schedule_over_recorded_schedule=t["this_d"] / t["this_r"])
        print(cfg, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in summary[cfg].items() if not isinstance(v, dict)}), flush=True)
    if record.get("bench"):
        val = {who: [b["value"] for b in record["bench"] if b["who"] == who] for who in ("this", "parent")}
        med = {who: statistics.median(v) for who, v in val.items()}
        spread = max((max(v) - min(v)) / statistics.median(v) for v in val.values())
        summary["bench"] = dict(value_median=med, values=val, largest_spread_reported=spread, this_over_parent=med["this"] / med["parent"],
                                agrees_within_3_spreads=abs(med["this"] / med["parent"] - 1.0) <= 3.0 * spread)
        print("bench", json.dumps(summary["bench"]), flush=True)
    return summary


def bench_line(root, steps, warmup, timeout):
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-gather"],
                         cwd=root, capture_output=True, text=True, timeout=timeout)
    for ln in reversed(out.stdout.splitlines()):
        if ln.startswith("{") and '"value"' in ln:
            d = json.loads(ln)
            return dict(value=d["value"], unit=d.get("unit"), ms_per_step=d.get("ms_per_step"), timing=d.get("config", {}).get("timing"))
    raise SystemExit("dt_schedule_rate: no result line from %s/bench.py\n%s\n%s" % (root, out.stdout[-2000:], out.stderr[-2000:]))


def versus(args):
    parent = os.path.abspath(args.versus)
    record = {"tool": "tools/dt_schedule_rate.py --versus", "rounds": [], "bench": [],
              "note": "every entry is a fresh process; 'this' (d, D, s, r, p, f) and 'parent' (p, f) alternate.  d, D, p and f are effective "
                      "figures (temporal fusion: the state stays in registers over the call's 20 ticks).  PMC bytes were not collected."}
    for rnd in range(args.rounds):
        for who, root, forms in (("this", ROOT, ALL), ("parent", parent, OLD)):
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--root", root, "--forms", forms, "--out", tmp.name, "--seconds",
                                       str(args.seconds), "--reps", str(args.reps), "--configs", args.configs], timeout=args.child_timeout)
                rec = json.load(open(tmp.name))
                rec["root"] = who
                record["rounds"].append({"round": rnd, "who": who, "record": rec})
        if args.bench_steps > 0:
            for who, root in (("this", ROOT), ("parent", parent)):
                record["bench"].append(dict(round=rnd, who=who, **bench_line(root, args.bench_steps, args.bench_warmup, args.child_timeout)))
    record["summary"] = summarise(record, args.configs.split(","))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="uv_1e4,ar_1e6")
    ap.add_argument("--forms", default=ALL, help="d = fused schedule, D = fused gated schedule, s = eager schedule sequence, r = the same as a recorded "
                                                 "graph, p = plain step_fused (scalar dt), f = fused gate (scalar dt)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are measured (default: this one)")
    ap.add_argument("--versus", default=None, help="another checkout (the parent commit, built): alternate fresh processes of both")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=0, help="with --versus: also alternate bench.py --gpus 1 --steps K of both checkouts (0: no)")
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--child-timeout", type=float, default=280.0)
    ap.add_argument("--summarise-from", default=None, help="a --versus record: recompute its summary from its rounds (no GPU) and write it to --out")
    args = ap.parse_args()
    if args.summarise_from:
        record = json.load(open(args.summarise_from))
        record["summary"] = summarise(record, args.configs.split(","))
        with open(args.out or args.summarise_from, "w") as f:
            json.dump(record, f, indent=1)
        return None
    if args.versus:
        return versus(args)
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dt_schedule_rate: needs a GPU")
    import numpy as np
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    forms = [f for f in ALL if f in args.forms]
    sched = DT * np.random.default_rng(SEED).uniform(0.25, 2.0, TICKS)
    record = {"tool": "tools/dt_schedule_rate.py", "nis_max": GAMMA, "max_rejects": K, "ticks_per_call": TICKS, "device": torch.cuda.get_device_name(0),
              "schedule_over_dt": list(sched / DT), "forms": {f: NAMES[f] for f in forms}, "configs": {}}
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
        gated = dict(innov=(nis, None), gate=GAMMA, reacquire=(K, events))

        def call(f):
            b = mgrs[f][1]
            if f == "d":
                b.step_fused(sched, meas)
            elif f == "D":
                b.step_fused(sched, meas, **gated)
            elif f == "p":
                b.step_fused(DT, meas)
            elif f == "f":
                b.step_fused(DT, meas, **gated)
            else:
                b.step_sequence(sched, meas, use_graph=(f == "r"))

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
        if "d" in forms:
            out["fused_dt_served"] = [int(mgrs["d"][1].fused_dt_served(False)), int(mgrs["D"][1].fused_dt_served(True)) if "D" in forms else None]
        if "r" in forms:
            out["recordings_of_the_recorded_form"] = int(mgrs["r"][1].graph_recordings)
        for rep in range(args.reps):
            for f in (forms if rep % 2 == 0 else forms[::-1]):
                res[f].append(dict(tick_us=timed(f, calls[f]) / (calls[f] * TICKS) * 1e6, calls=calls[f]))
        torch.cuda.synchronize()
        for f in forms:
            t = [r["tick_us"] for r in res[f]]
            med = statistics.median(t)
            out["forms"][f] = dict(reps=res[f], tick_us_median=med, tick_us_min=min(t), tick_us_max=max(t), spread=(max(t) - min(t)) / med,
                                   effective=f in EFFECTIVE)
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
