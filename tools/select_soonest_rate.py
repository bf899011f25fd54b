#!/usr/bin/env python3
"""The k soonest sphere crossings of a manager: the library's selection (TargetManager.select_soonest, device form) against the two
ways the same job is done without it (GPU only).  Shapes, each right after a tick with the query:
  cfg4_1m     500 000 angular-rates + 500 000 uniform-acceleration targets, fp32, one GPU (BASELINE configs[4]'s population)
  small_1e4   5 000 + 5 000 of the same models
each with k = 8 and k = 256, `plain` (no mask, no pose gather) and `full` (the convergence gate's mask and the pose gather).  Forms:
  (s) selection   ONE TargetManager.select_soonest(..., device=True) per call: three launches, result left on the device
  (a) host        a synchronising copy of every batch's delta (and mask) to the host, numpy.argpartition and a sort of the k
  (b) torch.topk  torch.topk(..., largest=False) on the masked device tensor (the batches' deltas concatenated), then the gather
                  of the poses
HIP events around each timed region for s and b; form a synchronises by itself and is timed on the host clock.  A warm-up per
variant, --reps repetitions per process; the forms run in FRESH PROCESSES that alternate (--rounds of s, a, b).  The record keeps
every repetition, the median per process and the spread ((max - min) / median over a process's repetitions).  The s processes also
time the tick itself (step_sequence_all, one tick, query fused) and report the selection as a share of it.  HBM-side bytes (PMC)
are not collected.
  python tools/select_soonest_rate.py --out profiles/select_soonest_rate.json [--seconds 0.1] [--reps 3] [--rounds 3]
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
SHAPES = {"cfg4_1m": [("angular_rates", 500_000), ("uniform_acceleration", 500_000)],
          "small_1e4": [("angular_rates", 5_000), ("uniform_acceleration", 5_000)]}
VARIANTS = [(8, "plain"), (8, "full"), (256, "plain"), (256, "full")]
DT, SEED, ORIGIN, RADIUS = 0.004, 20240023, (0.0, 0.0, 0.0), 5.0   # the generator starts targets in [-10, 10]^3: most are outside and some head for the sphere
NAMES = {"s": "library selection (device form)", "a": "copy to the host + numpy.argpartition", "b": "torch.topk + pose gather"}


def drive(args):
    record = {"tool": "tools/select_soonest_rate.py", "rounds": [],
              "note": "every entry is a fresh process; the forms s, a, b alternate.  Times per call in microseconds.  PMC bytes were not collected."}
    orders = ["sab", "bsa", "abs"]
    for rnd in range(args.rounds):
        for form in orders[rnd % 3]:
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--form", form, "--out", tmp.name, "--seconds", str(args.seconds),
                                       "--reps", str(args.reps), "--shapes", args.shapes], timeout=args.child_timeout)
                record["rounds"].append({"round": rnd, "form": form, "record": json.load(open(tmp.name))})
    summary = {}
    for shape in args.shapes.split(","):
        for k, mode in VARIANTS:
            key = "%s_k%d_%s" % (shape, k, mode)
            per = {f: [r["record"]["shapes"][key] for r in record["rounds"] if r["form"] == f] for f in "sab"}
            med = {f: statistics.median(x["call_us_median"] for x in per[f]) for f in "sab"}
            spread = max(x["spread"] for f in "sab" for x in per[f])
            tick = statistics.median(x["tick_us_median"] for x in per["s"])
            summary[key] = dict(selection_us=med["s"], host_copy_us=med["a"], topk_us=med["b"], host_over_selection=med["a"] / med["s"],
                                topk_over_selection=med["b"] / med["s"], tick_us=tick, selection_share_of_tick=med["s"] / tick,
                                per_process={f: [x["call_us_median"] for x in per[f]] for f in "sab"}, largest_spread_reported=spread,
                                margin=3.0 * spread, selection_faster_than_host_beyond_margin=med["a"] / med["s"] > 1.0 + 3.0 * spread)
            print(key, json.dumps({k2: (round(v, 4) if isinstance(v, float) else v) for k2, v in summary[key].items() if not isinstance(v, dict)}), flush=True)
    record["summary"] = summary
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--form", default=None, help="s, a or b: measure that form in this process (the driver starts these)")
    ap.add_argument("--child-timeout", type=float, default=200.0)
    args = ap.parse_args()
    if args.reps < 3 or args.rounds < 1:
        raise SystemExit("select_soonest_rate: at least 3 repetitions")
    if args.form is None:
        return drive(args)
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("select_soonest_rate: needs a GPU")
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

    def events(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def host_clock(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return time.perf_counter() - t0

    def measure(fn, timer):
        for _ in range(3):
            fn()
        calls = max(3, int(args.seconds / (timer(fn, 3) / 3)))
        t = [timer(fn, calls) / calls * 1e6 for _ in range(args.reps)]
        med = statistics.median(t)
        return dict(reps_us=t, calls=calls, median=med, spread=(max(t) - min(t)) / med)

    record = {"tool": "tools/select_soonest_rate.py", "form": form, "form_name": NAMES[form], "device": torch.cuda.get_device_name(0), "shapes": {}}
    ticks = 4
    for shape in args.shapes.split(","):
        parts = SHAPES[shape]
        mgr = te.TargetManager(dtype="f32")
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        meas, base = [], 0
        for j, (name, n) in enumerate(parts):
            mdl = model_params(name)
            st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, SEED + 17 * j, dtype="f32")
            ids = np.arange(n, dtype=np.uint32) + base
            base += n
            assert mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=mdl["Q"], R=mdl["R"], P0=mdl["P"]) == n
            meas.append(st["meas"])
        bs = mgr.batches()
        deltas = [torch.empty(b.size, dtype=torch.float64, device="cuda") for b in bs]
        poses = [torch.empty((b.size, 7), dtype=torch.float64, device="cuda") for b in bs]
        query = (ORIGIN, RADIUS, deltas, poses)
        # A few ticks with the query and the gate, so that delta, pose and the mask are what a node loop holds.  A gate's first position
        # error is the distance from its initial pose [0 0 0] to the sphere, so the window is 2 ticks and has forgotten it by the third;
        # the last tick's threshold is the median of the filtered errors one tick earlier: about half of the crossings converge.
        masks, pos_th = None, 1e9
        for s in range(ticks):
            mgr.step_sequence_all(DT, [m[s:s + 1] for m in meas], query=query, use_graph=False)
            res = [b.gate_update(d, p, pos_th, 1e9, filters_length=2) for b, d, p in zip(bs, deltas, poses)]
            masks = [r[0] for r in res]
            if s == ticks - 2:
                pos_th = float(torch.cat([r[1][d >= 0, 0] for r, d in zip(res, deltas)]).median().item())
        torch.cuda.synchronize()
        crossing = int(sum((d >= 0).sum().item() for d in deltas))
        converged = int(sum(((d >= 0) & (m != 0)).sum().item() for d, m in zip(deltas, masks)))
        if not (crossing <= 4 * converged and converged < crossing):   # a substantial part of the crossings, and not all of them
            raise SystemExit("select_soonest_rate: %s: %d of %d crossings converged -- the `full` shapes would not time a masked selection of "
                             "k rows; nothing recorded" % (shape, converged, crossing))
        tick = measure(lambda: mgr.step_sequence_all(DT, [m[ticks - 1:ticks] for m in meas], query=query, use_graph=False), events) if form == "s" else None
        for k, mode in VARIANTS:
            full = mode == "full"
            ok = masks if full else None
            if form == "s":
                out = mgr.select_soonest((deltas, poses), ok=ok, k=k, want_pose=full, device=True)
                res = measure(lambda: mgr.select_soonest((deltas, poses), ok=ok, k=k, want_pose=full, device=True, out=out), events)
            elif form == "a":
                def host():
                    d = np.concatenate([x.cpu().numpy() for x in deltas])
                    keep = d >= 0.0
                    if full:
                        keep &= np.concatenate([x.cpu().numpy() for x in masks]) != 0
                    d = np.where(keep, d, np.inf)
                    kk = min(k, len(d) - 1)
                    idx = np.argpartition(d, kk)[:k]
                    return idx[np.argsort(d[idx], kind="stable")]
                res = measure(host, host_clock)
            else:
                inf = torch.tensor(float("inf"), dtype=torch.float64, device="cuda")

                def topk():
                    d = torch.cat(deltas)
                    keep = d >= 0.0
                    if full:
                        keep &= torch.cat(masks) != 0
                    v, idx = torch.topk(torch.where(keep, d, inf), k, largest=False)
                    if not full:
                        return v, idx
                    n0 = deltas[0].numel()   # (the k rows are gathered from the batch each lies in: no copy of the pose arrays)
                    rows = torch.where((idx < n0)[:, None], poses[0][idx.clamp(max=n0 - 1)], poses[1][(idx - n0).clamp(min=0)])
                    return v, idx, rows
                res = measure(topk, events)
            out = dict(parts=parts, k=k, mode=mode, form=form, crossing=crossing, converged=converged, reps_us=res["reps_us"], calls=res["calls"],
                       call_us_median=res["median"], spread=res["spread"])
            if tick is not None:
                out.update(tick_us_median=tick["median"], tick_spread=tick["spread"], tick_reps_us=tick["reps_us"])
            record["shapes"]["%s_k%d_%s" % (shape, k, mode)] = out
            print(shape, k, mode, NAMES[form], round(res["median"], 2), "us per call, spread", round(res["spread"], 4), flush=True)
        mgr.close()
        del meas, deltas, poses, masks
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
