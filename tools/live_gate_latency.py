#!/usr/bin/env python3
"""What the gate costs a resident tick: the paced per-tick latency (one doorbell, spin until the tick is done, next doorbell --
the way profiles/r04_bar_doorbell.txt was taken, through the Python binding) of a GATED session with NIS and event rows and the
gate at +inf (K = 3: every measurement is accepted, the whole gated body and both row stores run) against the POSE-OUTPUT session
(kLive2) of the same batch, whose kernel this library has from its parent unchanged.
    10^4 uniform-velocity f64 targets                          BASELINE configs[1]
    62 500 angular-rates + 62 500 angular-velocities, f64     configs[3]'s share of one device, both resident together
The two kinds of session alternate, REPS sessions each, WARM + PACED ticks per session; per kind the median of the sessions'
medians and the spread (min .. max of them).  Behind them the capacities the occupancy query grants the gated kernels, in the
format of tools/live_capacity.py.
    python tools/live_gate_latency.py [--reps 5] [--paced 3000]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = {"angular_rates": 0, "angular_velocities": 1, "uniform_acceleration": 2, "uniform_velocity": 3}
CASES = [(m, d) for m in ("uniform_velocity", "uniform_acceleration", "angular_rates", "angular_velocities") for d in ("f64", "f32")]
DT, RING, WARM = 0.004, 64, 200


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def session(parts, dtype, gated, paced):
    """one session over `parts` = [(model name, targets), ...]: the sorted per-tick microseconds of `paced` paced ticks"""
    import torch
    import target_estimation_amd as te
    from target_estimation_amd.streams import make_stream
    import yaml
    stream = torch.cuda.Stream()
    mgr = te.TargetManager(dtype=dtype)
    mgr.set_stream(stream.cuda_stream)
    rings, keep, base = [], [], 0
    for k, (name, n) in enumerate(parts):
        with open(os.path.join(ROOT, "models", "model_%s_params.yaml" % name)) as f:
            node = yaml.safe_load(f)
        ns, nm = te.manager.MODEL_DIMS[MODELS[name]]
        mdl = dict(model=MODELS[name], Q=np.array(node["Q"], dtype=np.float64).reshape(ns, ns), R=np.array(node["R"], dtype=np.float64).reshape(nm, nm),
                   P=np.array(node["P"], dtype=np.float64).reshape(ns, ns))
        st = make_stream(MODELS[name], n, RING, DT, 5 + k, dtype=dtype)
        mgr.init_batch(np.arange(n, dtype=np.uint32) + base, DT, 0.0, st["p0"].cpu().numpy(), type=mdl["model"], Q=mdl["Q"], R=mdl["R"], P0=mdl["P"])
        base += n
        rings.append(st["meas"])
    for b in mgr.batches():
        n = b.size
        if gated:
            nis = torch.zeros((RING, n), dtype=torch.float64, device="cuda")
            ev = torch.zeros((RING, n), dtype=torch.uint8, device="cuda")
            b.live_set_gate(float("inf"), nis, reacquire=(3, ev))
            keep += [nis, ev]
        else:
            pose = torch.zeros((7, n), dtype=torch.float64, device="cuda")
            b.live_set_pose_output(pose)
            keep.append(pose)
    torch.cuda.synchronize()
    mgr.live_start_all(DT, rings, max_ticks=WARM + paced, idle_limit_s=3.0)
    us = np.zeros(paced)
    try:
        for i in range(WARM + paced):
            t0 = time.perf_counter()
            mgr.live_post_all(1)
            if not mgr.live_wait_all(i + 1, 5.0):
                raise RuntimeError("tick %d was not served" % i)
            if i >= WARM:
                us[i - WARM] = (time.perf_counter() - t0) * 1e6
    finally:
        served = mgr.live_stop_all()
    assert served == WARM + paced, served
    mgr.close()
    return np.sort(us)


def main():
    import torch
    import target_estimation_amd as te
    reps, paced = arg("--reps", 5), arg("--paced", 3000)
    print("# paced per-tick latency, us: median of %d sessions' medians [min .. max of them]; %d paced ticks per session behind %d warm ones" % (reps, paced, WARM))
    for what, parts, dtype in (("10000 uniform_velocity f64 (configs[1])", [("uniform_velocity", 10000)], "f64"),
                               ("62500 angular_rates + 62500 angular_velocities f64 (configs[3]'s share)",
                                [("angular_rates", 62500), ("angular_velocities", 62500)], "f64"),
                               ("50000 angular_rates + 50000 angular_velocities f64 (the largest round share both gated kernels hold together)",
                                [("angular_rates", 50000), ("angular_velocities", 50000)], "f64")):
        try:   # (a population the gated kernels cannot hold together is refused at the start: said, and the next size is taken)
            session(parts, dtype, True, 10)
        except RuntimeError as e:
            print("%s\n  gated session REFUSED: %s" % (what, str(e)[-160:]), flush=True)
            continue
        med = {False: [], True: []}
        for _ in range(reps):
            for gated in (False, True):   # alternating
                med[gated].append(float(np.median(session(parts, dtype, gated, paced))))
        p, g = np.median(med[False]), np.median(med[True])
        print("%s" % what)
        print("  pose-output session (kLive2)       %6.2f  [%6.2f .. %6.2f]" % (p, min(med[False]), max(med[False])))
        print("  gated session, gate +inf, K = 3    %6.2f  [%6.2f .. %6.2f]" % (g, min(med[True]), max(med[True])))
        print("  ratio gated / pose-output          %6.3f" % (g / p), flush=True)
    print("# capacities (targets) of the resident kernels: target_batch_live_capacity plain / with the pose output / with a gate set")
    for name, dtype in CASES:
        m = te.TargetManager(os.path.join(ROOT, "models", "model_%s_params.yaml" % name), dtype=dtype)
        p0 = np.zeros((64, 7)); p0[:, 6] = 1.0
        m.init_batch(np.arange(64, dtype=np.uint32), DT, 0.0, p0)
        b = m.batches()[0]
        plain = b.live_capacity
        buf = torch.zeros((7, 64), dtype=torch.float64, device="cuda")
        b.live_set_pose_output(buf)
        with_out = b.live_capacity
        b.live_set_pose_output(None)
        b.live_set_gate(float("inf"), torch.zeros((1, 64), dtype=torch.float64, device="cuda"), reacquire=(3, None))
        gated = b.live_capacity
        m.close()
        print("%-22s %s  plain %7d   with query / pose output %7d   gated %7d" % (name, dtype, plain, with_out, gated), flush=True)


if __name__ == "__main__":
    main()
