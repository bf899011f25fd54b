#!/usr/bin/env python3
"""What uniform tiles cost where they do not apply (GPU only).  10^6 angular_rates targets, fp64, eager dense ticks over a ring
of 16 ticks of measurements, HIP events around each timed region:
  masked   a 90 % availability mask: no tile stays uniform, so every wavefront pays the flag load its covariance-chunk loads
           wait for, and a promoting tick the comparison of its lanes
  by_id    a fresh population, unmasked, with one by-id update (the reference's one-target call) between every 8 dense ticks: a settle pass, the
           indexed launch and the re-promotion behind the gate, every 8 ticks
Variants alternate inside one process, --reps times: `on` / `off` = managers with uniform_tiles=True / False.  `default` builds
the manager without the keyword, for a checkout that predates it: run the tool from that checkout with --package-root.
  python tools/uniform_tiles_nonuniform.py --variants on,off [--seconds 0.5] [--reps 4]
  python tools/uniform_tiles_nonuniform.py --variants default --package-root /path/to/parent/checkout
One JSON line per (case, variant, repetition) and one with the medians."""
import argparse
import json
import os
import statistics
import sys

N, RING, DT, SEED = 1_000_000, 16, 0.004, 20240008


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="on,off")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("uniform_tiles_nonuniform: needs a GPU")
    import numpy as np
    import yaml
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    name = "angular_rates"
    with open(os.path.join(args.package_root, "models", "model_%s_params.yaml" % name)) as f:
        node = yaml.safe_load(f)
    ns, nm = te.MODEL_DIMS[te.MODEL_TYPES[name]]
    Q, R, P = (np.array(node[k], dtype=np.float64).reshape(d, d) for k, d in (("Q", ns), ("R", nm), ("P", ns)))
    st = make_stream(te.MODEL_TYPES[name], N, RING, DT, SEED, availability=0.9)
    meas, has = st["meas"], st["has_meas"]
    ids = np.arange(N, dtype=np.uint32)
    row = meas[0, :, 5].cpu().numpy().copy()
    variants = args.variants.split(",")

    def populations():   # a fresh population per case: after masked ticks the lanes of a tile differ, and nothing would promote again
        mgrs = {}
        for v in variants:
            kw = {} if v == "default" else dict(uniform_tiles=(v == "on"))
            m = te.TargetManager(dtype="f64", **kw)
            m.set_stream(torch.cuda.current_stream().cuda_stream)
            assert m.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=Q, R=R, P0=P) == N
            mgrs[v] = m
        return mgrs

    def masked(m, b, blocks):
        for _ in range(blocks):
            b.step_sequence(DT, meas, has)
        return blocks * RING

    def by_id(m, b, blocks):
        for _ in range(blocks):
            b.step_sequence(DT, meas[:8])
            m.update(5, DT, row)
            b.step_sequence(DT, meas[8:])
            m.update(5, DT, row)
        return blocks * RING

    def timed(fn, m, b, blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ticks = fn(m, b, blocks)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ticks   # ms per dense tick

    results = {}
    for case, fn in (("masked", masked), ("by_id", by_id)):
        mgrs = populations()
        blocks = {}
        for v in variants:   # warm-up, and the number of blocks that fills --seconds
            b = mgrs[v].batches()[0]
            timed(fn, mgrs[v], b, 2)
            ms = timed(fn, mgrs[v], b, 4)
            blocks[v] = max(4, int(args.seconds * 1e3 / (ms * RING)))
        for rep in range(args.reps):
            for v in variants:
                b = mgrs[v].batches()[0]
                ms = timed(fn, mgrs[v], b, blocks[v])
                tiles = getattr(b, "uniform_tiles", None)
                results.setdefault((case, v), []).append(ms)
                print(json.dumps(dict(label=args.label, case=case, variant=v, rep=rep, ms_per_tick=round(ms, 6), uniform_tiles_after=tiles)), flush=True)
        for m in mgrs.values():
            m.close()
    print(json.dumps(dict(label=args.label, medians={"%s/%s" % k: round(statistics.median(v), 6) for k, v in results.items()},
                          spread={"%s/%s" % k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in results.items()})), flush=True)


if __name__ == "__main__":
    main()
