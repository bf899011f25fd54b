#!/usr/bin/env python3
"""Position covariance and time spread at the sphere crossings: the library's call (Batch.crossing_cov / TargetManager.crossing_cov,
device forms) against doing the same without it -- target_manager_get_state_batch of the ids in question plus NumPy (GPU only).
Population: 500 000 angular-rates + 500 000 uniform-acceleration targets, fp32, one GPU (BASELINE configs[4]), right after a tick
with the query.  Measured:
  dense       one Batch.crossing_cov per batch over all 10^6 deltas (cov, sigma, ok); most targets do not cross and cost their delta
  rows_k8     TargetManager.crossing_cov on the 8 rows TargetManager.select_soonest(device=True) left on the device
  rows_k256   the same for 256 rows
Forms:
  (c) the library call, HIP events around `calls` back-to-back calls
  (h) the alternative on the host clock (it synchronises by itself): get_state_batch of the same ids, batch by batch, then
      Sigma = (A(tau) P A(tau)^T + Q)[0:3, 0:3] and sigma_r / sigma_t in NumPy.  For `dense` the ids are those of the crossers only
      (the alternative's best case: it already knows who crosses).
A warm-up per shape, --reps repetitions per process; the forms run in FRESH PROCESSES that alternate (--rounds of c, h).  The record
keeps every repetition, the median per process and the spread ((max - min) / median over a process's repetitions).  The c processes
also time the tick itself (step_sequence_all, one tick, query fused) and report each call as a share of it.
  python tools/crossing_cov_rate.py --out profiles/crossing_cov_rate.json [--seconds 0.1] [--reps 3] [--rounds 3]
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
PARTS = [("angular_rates", 500_000), ("uniform_acceleration", 500_000)]
SHAPES = ["dense", "rows_k8", "rows_k256"]
DT, SEED, ORIGIN, RADIUS = 0.004, 20240023, (0.0, 0.0, 0.0), 5.0   # the generator starts targets in [-10, 10]^3: most are outside and some head for the sphere
NAMES = {"c": "library call (device form)", "h": "get_state_batch of the ids + NumPy"}


def drive(args):
    record = {"tool": "tools/crossing_cov_rate.py", "rounds": [],
              "note": "every entry is a fresh process; the forms c, h alternate.  Times per call in microseconds."}
    for rnd in range(args.rounds):
        for form in ("ch", "hc")[rnd % 2]:
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--form", form, "--out", tmp.name, "--seconds", str(args.seconds),
                                       "--reps", str(args.reps), "--scale", str(args.scale)], timeout=args.child_timeout)
                record["rounds"].append({"round": rnd, "form": form, "record": json.load(open(tmp.name))})
    summary = {}
    for shape in SHAPES:
        per = {f: [r["record"]["shapes"][shape] for r in record["rounds"] if r["form"] == f] for f in "ch"}
        med = {f: statistics.median(x["call_us_median"] for x in per[f]) for f in "ch"}
        spread = max(x["spread"] for f in "ch" for x in per[f])
        tick = statistics.median(x["tick_us_median"] for x in per["c"])
        summary[shape] = dict(call_us=med["c"], host_us=med["h"], host_over_call=med["h"] / med["c"], tick_us=tick, call_share_of_tick=med["c"] / tick,
                              host_share_of_tick=med["h"] / tick, rows=per["c"][0]["rows"], candidates=per["c"][0]["candidates"],
                              per_process={f: [x["call_us_median"] for x in per[f]] for f in "ch"}, largest_spread_reported=spread)
        print(shape, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in summary[shape].items() if not isinstance(v, dict)}), flush=True)
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
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the population (a trial run of the tool itself)")
    ap.add_argument("--form", default=None, help="c or h: measure that form in this process (the driver starts these)")
    ap.add_argument("--child-timeout", type=float, default=200.0)
    args = ap.parse_args()
    if args.reps < 3 or args.rounds < 1:
        raise SystemExit("crossing_cov_rate: at least 3 repetitions")
    if args.form is None:
        return drive(args)
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("crossing_cov_rate: needs a GPU")
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

    record = {"tool": "tools/crossing_cov_rate.py", "form": form, "form_name": NAMES[form], "device": torch.cuda.get_device_name(0), "shapes": {}}
    ticks = 4
    mgr = te.TargetManager(dtype="f32")
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    meas, base, mdl = [], 0, []
    for j, (name, n) in enumerate(PARTS):
        n = max(64, int(n * args.scale))
        mdl.append(model_params(name))
        st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, SEED + 17 * j, dtype="f32")
        ids = np.arange(n, dtype=np.uint32) + base
        base += n
        assert mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=mdl[j]["Q"], R=mdl[j]["R"], P0=mdl[j]["P"]) == n
        meas.append(st["meas"])
    bs = mgr.batches()
    deltas = [torch.empty(b.size, dtype=torch.float64, device="cuda") for b in bs]
    poses = [torch.empty((b.size, 7), dtype=torch.float64, device="cuda") for b in bs]
    query = (ORIGIN, RADIUS, deltas, poses)
    for s in range(ticks):
        mgr.step_sequence_all(DT, [m[s:s + 1] for m in meas], query=query, use_graph=False)
    torch.cuda.synchronize()
    hd = [d.cpu().numpy() for d in deltas]
    crossing = int(sum((d >= 0).sum() for d in hd))
    origin = np.array(ORIGIN)

    def numpy_rows(b, j, ids, tau):
        """get_state_batch of one batch's ids, then Sigma, sigma_r, sigma_t as the kernel defines them"""
        if len(ids) == 0:
            return None
        x, P = mgr.get_state_batch(ids)
        K = te.MODEL_DIMS[te.MODEL_TYPES[PARTS[j][0]]][1]
        coef = np.stack([np.ones_like(tau), tau, 0.5 * tau * tau], axis=1)                      # both models carry [p v a] chains
        Sg = np.empty((len(ids), 3, 3))
        for r in range(3):
            for c in range(3):
                blk = P[:, r::K, c::K][:, :3, :3]
                Sg[:, r, c] = np.einsum("ni,nij,nj->n", coef, blk, coef) + mdl[j]["Q"][r, c]
        pc = np.stack([(coef * x[:, r::K][:, :3]).sum(axis=1) for r in range(3)], axis=1)
        vc = np.stack([x[:, r + K] + x[:, r + 2 * K] * tau for r in range(3)], axis=1)
        d = pc - origin
        nrm = d / np.linalg.norm(d, axis=1, keepdims=True)
        sr = np.sqrt(np.einsum("ni,nij,nj->n", nrm, Sg, nrm))
        return Sg, sr, sr / np.abs((nrm * vc).sum(axis=1))

    for shape in SHAPES:
        if shape == "dense":
            rows = sum(b.size for b in bs)
            if form == "c":
                outs = [b.crossing_cov(d, origin=ORIGIN, radius=RADIUS, sigma_t_max=0.002) for b, d in zip(bs, deltas)]

                def call():
                    for b, d, o in zip(bs, deltas, outs):
                        b.crossing_cov(d, origin=ORIGIN, radius=RADIUS, sigma_t_max=0.002, out=o)
                res = measure(call, events)
            else:
                sel = [np.flatnonzero(d >= 0) for d in hd]
                sids = [b.slot_ids() for b in bs]

                def host():
                    return [numpy_rows(b, j, sids[j][sel[j]], hd[j][sel[j]]) for j, b in enumerate(bs)]
                res = measure(host, host_clock)
        else:
            k = int(shape.split("k")[1])
            rows = k
            cnt, bo, so, do, po = mgr.select_soonest((deltas, poses), k=k, want_pose=False, device=True)
            torch.cuda.synchronize()
            if form == "c":
                out = mgr.crossing_cov(bo, so, do, origin=ORIGIN, radius=RADIUS, sigma_t_max=0.002)
                res = measure(lambda: mgr.crossing_cov(bo, so, do, origin=ORIGIN, radius=RADIUS, sigma_t_max=0.002, out=out), events)
            else:
                count = int(cnt.item())
                hb, hs, hdl = bo.cpu().numpy()[:count], so.cpu().numpy()[:count], do.cpu().numpy()[:count]
                sids = [b.slot_ids() for b in bs]

                def host():
                    return [numpy_rows(b, j, sids[j][hs[hb == j]], hdl[hb == j]) for j, b in enumerate(bs)]
                res = measure(host, host_clock)
        out_rec = dict(shape=shape, form=form, rows=rows, candidates=crossing, targets=sum(b.size for b in bs), reps_us=res["reps_us"], calls=res["calls"],
                       call_us_median=res["median"], spread=res["spread"])
        record["shapes"][shape] = out_rec
        print(shape, NAMES[form], round(res["median"], 2), "us per call, spread", round(res["spread"], 4), flush=True)
    if form == "c":      # the tick itself, LAST: its timed repetitions move the state on, and both forms must see the same crossings above
        tick = measure(lambda: mgr.step_sequence_all(DT, [m[ticks - 1:ticks] for m in meas], query=query, use_graph=False), events)
        for out_rec in record["shapes"].values():
            out_rec.update(tick_us_median=tick["median"], tick_spread=tick["spread"], tick_reps_us=tick["reps_us"])
    mgr.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
