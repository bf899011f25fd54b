#!/usr/bin/env python3
"""What sharding one manager costs on one device, and what target_manager_get_est_all_by_id achieves (GPU only).
  (1) the population tick of cfg4_1gpu (500 000 angular-rates + 500 000 angular-velocities, fp64) on 1, 2, 4 and 8 logical
      shards on device 0 (target_manager_set_devices), eager target_manager_step_sequence_all over a measurement ring, with and
      without a pose stream per batch;
  (2) target_manager_get_est_all_by_id on the same 10^6 targets into device memory and into pinned host memory, ids created in
      order and permuted at random, against target_batch_get_est_dev per batch (slot order, device memory).
HIP events around each timed region, a warm-up per form, forms alternated and repeated (--reps); the record keeps every
repetition and the median.
  python tools/shard_rate.py --out profiles/r06_shard_rate.json [--reps 3] [--ticks 64] [--shards 1,2,4,8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POP = [("angular_rates", 500_000), ("angular_velocities", 500_000)]
RING, DT = 16, 0.004


def build(te, np, devices, permuted):
    def model_path(name):
        return os.path.join(ROOT, "models", "model_%s_params.yaml" % name)
    m = te.TargetManager(model_path(POP[0][0]), devices=devices)
    n = sum(k for _, k in POP)
    ids = np.arange(1, n + 1, dtype=np.uint32)
    if permuted:
        ids = np.random.default_rng(7).permutation(ids)
    p0 = np.zeros((n, 7)); p0[:, 6] = 1.0
    m.init_batch(ids[:POP[0][1]], DT, 0.0, p0[:POP[0][1]])
    q = te.TargetManager(model_path(POP[1][0]))
    q.init(1, DT, 0.0, [0, 0, 0, 0, 0, 0, 1])
    Q, R, P0 = q.getModelMatrices(1)
    q.close()
    m.init_batch(ids[POP[0][1]:], DT, 0.0, p0[POP[0][1]:], type=te.ANGULAR_VELOCITIES, Q=Q, R=R, P0=P0)
    return m


def timed(torch, fn, reps_inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps_inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps_inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--shards", default="1,2,4,8")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("shard_rate: needs a GPU")
    import target_estimation_amd as te
    rec = {"population": "cfg4_1gpu: 500000 angular_rates + 500000 angular_velocities, fp64", "ticks_per_call": args.ticks,
           "tick_us": {}, "gather_us": {}}
    # (1) the population tick on k logical shards
    for k in [int(s) for s in args.shards.split(",")]:
        m = build(te, np, [0] * k, False)
        bs = m.batches()
        meas = [torch.zeros((RING, 7, b.size), dtype=torch.float64, device="cuda") for b in bs]
        for t in meas:
            t[:, 6] = 1.0
        poses = [torch.zeros((1, 7, b.size), dtype=torch.float64, device="cuda") for b in bs]
        forms = {"plain": lambda: m.step_sequence_all(DT, meas, use_graph=0, n_ticks=args.ticks),
                 "poses": lambda: m.step_sequence_all(DT, meas, use_graph=0, n_ticks=args.ticks, poses=poses)}
        for f in forms.values():
            f()
        runs = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                runs[name].append(1000.0 * timed(torch, f) / args.ticks)
        rec["tick_us"]["%d_shards" % k] = {name: {"runs": r, "median": statistics.median(r)} for name, r in runs.items()}
        rec["tick_us"]["%d_shards" % k]["population_tick"] = m.population_tick()
        print(k, "shards", {n: round(statistics.median(r), 1) for n, r in runs.items()}, flush=True)
        m.close()
        torch.cuda.empty_cache()
    # (2) the ascending-id gather against the slot-ordered getter per batch
    for permuted in (False, True):
        for k in (1, 3):
            m = build(te, np, None if k == 1 else [0] * k, permuted)
            n = m.size()
            dev = torch.empty((n, 7), dtype=torch.float64, device="cuda")
            pin = torch.empty((n, 7), dtype=torch.float64).pin_memory()
            bs = m.batches()
            slot = [torch.empty((b.size, 7), dtype=torch.float64, device="cuda") for b in bs]
            lib = m._lib

            def per_batch():
                for b, t in zip(bs, slot):
                    lib.target_batch_get_est_dev(b._h, t.data_ptr(), None, None, 0, 0.0)
            forms = {"by_id_device": lambda: m.get_est_all_by_id(dev), "by_id_pinned": lambda: m.get_est_all_by_id(pin),
                     "get_est_dev_per_batch": per_batch}
            for f in forms.values():
                f()
            runs = {name: [] for name in forms}
            for _ in range(args.reps):
                for name, f in forms.items():
                    runs[name].append(1000.0 * timed(torch, f, 10))
            key = "%s_ids_%d_shards" % ("permuted" if permuted else "in_order", k)
            rec["gather_us"][key] = {name: {"runs": r, "median": statistics.median(r),
                                            "GB_s": 56.0 * n / (statistics.median(r) * 1e3)} for name, r in runs.items()}
            print(key, {nm: round(statistics.median(r), 1) for nm, r in runs.items()}, flush=True)
            m.close()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
