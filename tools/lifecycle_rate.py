#!/usr/bin/env python3
"""The track lifecycle on the device (TargetManager.lifecycle) against the only way to do the same work without it: the
host-composed path -- the mask read back, counters kept per slot in NumPy, erase_batch of the stale ids, init_batch of the unmatched
rows (GPU only).  Both paths are fed the SAME synthetic association results, frame after frame, on two managers of the same
population: uniform_velocity fp64 from the model file, N targets, a frame of M detections of which 1 % are unmatched (and finite:
born), a mask in which 1 % of the slots are 0 with max_misses = 1 (retired).  The association itself and the tick are not part of
either column: the lifecycle is what is compared.  What the host path needs on top and the device path does not -- the host form of
associate, which reads 16 M + 16 bytes of per-detection rows back so that the unmatched rows are known on the host -- is reported
as bytes, not timed.
Per shape and path: wall time around the call (both paths wait on the host by design) and, for the device path, HIP events around it;
one warm frame, then `reps` timed frames, median and spread (max - min) / median; the bytes read back per call, computed from the
call's counts (device: three counts and the retired slots, 4 B each; host: the mask, 1 B per slot; both upload the erase's move lists).
Nothing is gated.   python tools/lifecycle_rate.py --out profiles/lifecycle_rate.json [--reps 5] [--scale s]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(10_000, 10_000), (100_000, 100_000), (1_000_000, 1_000_000)]
DT = 0.004


def _erase_moves(np, n, stale):
    """Batch::erase_slots given the ascending list: holes below the new size <- the survivors at or above it, in order"""
    new_n = n - len(stale)
    gone = np.zeros(n, dtype=bool)
    gone[stale] = True
    return new_n + np.nonzero(~gone[new_n:])[0], np.nonzero(gone[:new_n])[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the shapes (a trial run of the tool itself)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lifecycle_rate: needs a GPU")
    import target_estimation_amd as te
    model = os.path.join(ROOT, "models", "model_uniform_velocity_params.yaml")
    record = {"tool": "tools/lifecycle_rate.py", "device": torch.cuda.get_device_name(0), "retired_share": 0.01, "born_share": 0.01,
              "note": "times in microseconds, measured by this run; the byte counts are computed from the calls' own counts; the association "
                      "and the tick are in neither column",
              "shapes": []}
    for N, M in SHAPES:
        N, M = max(int(N * args.scale), 100), max(int(M * args.scale), 100)
        rng = np.random.default_rng(N + M)
        mgrs = [te.TargetManager(model), te.TargetManager(model)]
        ids0 = np.arange(N, dtype=np.uint32)
        p0 = np.zeros((N, 7)); p0[:, 6] = 1.0
        p0[:, 0], p0[:, 1], p0[:, 2] = ids0 % 100, (ids0 // 100) % 100, ids0 // 10000
        for m in mgrs:
            m.set_stream(torch.cuda.current_stream().cuda_stream)
            assert m.init_batch(ids0, DT, 0.0, p0) == N
        A, B = mgrs
        miss = np.zeros(N, dtype=np.uint8)      # the host path's counters, by slot
        hits = np.zeros(N, dtype=np.uint8)
        next_id = 2_000_000_000
        dev_wall, dev_events, host_wall, retired_n, born_n = [], [], [], [], []
        for frame in range(args.reps + 1):
            n = A.size()
            assert n == B.size()
            # the frame and its association results, the same for both paths
            has = np.ones(n, dtype=np.uint8)
            has[rng.permutation(n)[:n // 100]] = 0
            det = np.zeros((M, 7)); det[:, 6] = 1.0
            det[:, :3] = rng.uniform(0, 100, (M, 3))
            sod = rng.integers(0, n, M).astype(np.int32)
            sod[rng.permutation(M)[:M // 100]] = -1
            has_dev, det_dev, sod_dev = torch.from_numpy(has).cuda(), torch.from_numpy(det).cuda(), torch.from_numpy(sod).cuda()
            torch.cuda.synchronize()
            # ---- the device path
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = A.lifecycle(det_dev, SimpleNamespace(has_meas=[has_dev], slot_of_det=sod_dev), max_misses=1, birth_type="uniform_velocity",
                              first_id=next_id, t_birth=DT * (frame + 1), dt0=DT)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            # ---- the host-composed path: the mask back, counters by slot, erase_batch, init_batch of the unmatched rows
            b = B.batches()[0]
            slot_ids = b.slot_ids()                     # (the caller's own bookkeeping would hold this: not timed)
            unmatched = np.nonzero(sod < 0)[0]          # (the host form of associate returns it: not timed)
            t2 = time.perf_counter()
            has_back = has_dev.cpu().numpy()
            seen = has_back != 0
            miss = np.where(seen, 0, np.minimum(miss.astype(np.int16) + 1, 255)).astype(np.uint8)
            hits = np.where(seen, np.minimum(hits.astype(np.int16) + 1, 255), hits).astype(np.uint8)
            stale = np.nonzero(miss >= 1)[0]
            gone = slot_ids[stale]
            src, dst = _erase_moves(np, n, stale)
            miss[dst], hits[dst] = miss[src], hits[src]
            miss, hits = miss[:n - len(stale)], hits[:n - len(stale)]
            assert B.erase_batch(gone) == len(gone)
            rows = unmatched[np.isfinite(det[unmatched]).all(axis=1)]
            new_ids = next_id + np.arange(len(rows), dtype=np.uint32)
            assert B.init_batch(new_ids, DT, DT * (frame + 1), det[rows]) == len(rows)
            miss = np.concatenate([miss, np.zeros(len(rows), dtype=np.uint8)])
            hits = np.concatenate([hits, np.zeros(len(rows), dtype=np.uint8)])
            t3 = time.perf_counter()
            assert out.retired == len(gone) and out.born == len(rows) and np.array_equal(out.retired_ids, gone)
            assert np.array_equal(A.batches()[0].slot_ids(), B.batches()[0].slot_ids())
            next_id += len(rows)
            if frame > 0:      # (frame 0 is the warm one: scratch and staging grow there)
                dev_wall.append((t1 - t0) * 1e6)
                dev_events.append(e0.elapsed_time(e1) * 1e3)
                host_wall.append((t3 - t2) * 1e6)
                retired_n.append(int(out.retired))
                born_n.append(int(out.born))
        ma, ha = A.batches()[0].track_counts()
        assert np.array_equal(ma, miss) and np.array_equal(ha, hits)

        def col(v):
            med = statistics.median(v)
            return dict(us=v, us_median=med, spread=(max(v) - min(v)) / med)

        r = statistics.median(retired_n)
        row = dict(N=N, M=M, retired_per_call=retired_n, born_per_call=born_n,
                   device=dict(wall=col(dev_wall), hip_events=col(dev_events), bytes_read_back_per_call=int(4 * 3 + 4 * r)),
                   host_composed=dict(wall=col(host_wall), bytes_read_back_per_call=int(n),
                                      bytes_read_back_by_the_host_form_of_associate_not_timed=16 * M + 16,
                                      bytes_of_born_rows_uploaded_per_call=int(56 * statistics.median(born_n))))
        row["host_over_device_wall"] = row["host_composed"]["wall"]["us_median"] / row["device"]["wall"]["us_median"]
        record["shapes"].append(row)
        print(json.dumps(dict(N=N, M=M, device_wall_us=round(row["device"]["wall"]["us_median"], 1),
                              device_events_us=round(row["device"]["hip_events"]["us_median"], 1),
                              host_wall_us=round(row["host_composed"]["wall"]["us_median"], 1), retired=r, born=statistics.median(born_n),
                              ratio=round(row["host_over_device_wall"], 2))), flush=True)
        for m in mgrs:
            m.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
