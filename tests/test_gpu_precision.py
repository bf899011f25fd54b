"""Precision matrix: every kernel path, in both precisions, against the extended-precision (f80, long double) oracle.

The parity tests compare a kernel with the oracle in its OWN precision, at tolerances far above what either side errs by.
Here each path runs next to two CPU oracles on identical inputs -- the strict oracle in the kernel's precision and the f80
oracle -- and at ticks 1, 10, 100, 200 and 300 (and on the derived outputs and the sphere query) must satisfy

    err(kernel vs f80) <= K * err(same-precision oracle vs f80) + floor        K = 8, floor = 8 eps(dtype)
    err(kernel vs f80) <= CEIL[dtype]

err is the maximum over the batch of |dx| / max(1, |x|) and of |dP| / max|P| (infinity norms per target): a faithful
implementation in a precision errs by what the oracle in that precision errs by (tests/test_highprec_kat.py pins those
figures); a kernel that loses digits does not.  For f32 every input (p0, v0, a0, Q, R, P0, measurements) is rounded to f32
before any side sees it, so the three sides differ only in arithmetic.  `pytest -s` prints the measured ratio of every row.

Inputs (edge_inputs): synth_stream, plus positions of order 1e4 m on every fourth target, measured yaw spinning through +-pi
several times per second, pitch held within 6e-3 rad of +-pi/2 (the gimbal branches of quatToRpy; 5e-2 for angular velocities), per-target P0, and a
schedule with masked ticks, single predict-only ticks and a run of 50 predict-only ticks (ticks 151-200)."""
import os

import numpy as np
import pytest

import oracle
from conftest import HARNESS_ORDER, model_path, synth_stream
from test_highprec_kat import P_err, f32r, x_err

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from test_gpu_parity import LANES, coupled  # noqa: E402  (after the importorskip of torch)

DT = 2.0 ** -8                  # exact in both precisions
T = 300
CHECK = (1, 10, 100, 200, 300)  # after these many ticks
NMAX = 1025
K = 8.0
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
# f64: SURVEY 8(d) (x, P); the outputs as the tightened parity tolerance; the sphere query's delta and intersection point 1e-10
# (measured 1.6e-12: a root near a grazing classification is ill-conditioned in any precision).  f32: the worst kernel error
# over every row of the model on the MI355X (in brackets) x 5 to 8.
CEIL = {"f64": {name: dict(x=1e-12, P=1e-10, out=1e-11, ix=1e-10) for name in HARNESS_ORDER},
        "f32": {"uniform_velocity": dict(x=5e-5, P=3e-4, out=5e-5, ix=1e-4),            # 7.8e-6, 4.1e-5, 7.8e-6, (no query)
                "uniform_acceleration": dict(x=1.5e-4, P=3e-4, out=1.5e-4, ix=2e-5),    # 2.0e-5, 4.5e-5, 1.9e-5, 3.3e-6
                "angular_rates": dict(x=2e-4, P=5e-4, out=3e-3, ix=1.5e-2),             # 3.5e-5, 7.4e-5, 5.1e-4, 2.1e-3
                "angular_velocities": dict(x=1e-4, P=3e-3, out=5e-5, ix=1e-4)}}         # 1.3e-5, 5.2e-4, 8.8e-6, (no query)
THREADS = min(16, os.cpu_count() or 1)
ORIGIN, RADIUS = np.array([0.5, -0.3, 0.2]), 6.0

_cache = {}


def _quat(roll, pitch, yaw):
    """rpyToQuat (the oracle's and the NumPy twin's formula), vectorised, [.., 4] = x y z w."""
    p, t, s = roll / 2, pitch / 2, yaw / 2
    c, n = np.cos, np.sin
    return np.stack([n(p) * c(t) * c(s) - c(p) * n(t) * n(s), c(p) * n(t) * c(s) + n(p) * c(t) * n(s),
                     c(p) * c(t) * n(s) - n(p) * n(t) * c(s), c(p) * c(t) * c(s) + n(p) * n(t) * n(s)], -1)


def _edge_stream(name):
    """NMAX targets, T ticks (the first n targets of it are a stream of n targets): p0 [NMAX,7], meas [T,NMAX,7] f64."""
    if ("stream", name) not in _cache:
        seed = 101 + HARNESS_ORDER.index(name)
        p0, meas = synth_stream(name, NMAX, T, seed=seed, dt=DT)
        i = np.arange(NMAX)
        far = i % 4 == 1
        off = np.array([1.2e4, -0.7e4, 0.4e4])
        p0[far, :3] += off
        meas[:, far, :3] += off
        if name in ("angular_rates", "angular_velocities"):
            rng = np.random.default_rng(seed + 1)
            t = DT * np.arange(T + 1)[:, None]
            roll = rng.uniform(-0.5, 0.5, NMAX) + rng.uniform(-1, 1, NMAX) * t
            pitch = rng.uniform(-0.6, 0.6, NMAX) + 0.2 * np.sin(rng.uniform(1, 4, NMAX) * t)
            yaw = rng.uniform(-3, 3, NMAX) + rng.uniform(-1, 1, NMAX) * t
            # measured yaw through +-pi every 0.15 s (angular rates) or 0.5 s (angular velocities: at the faster spin its filter
            # loses the target, and f64 and f80 part ways chaotically)
            spin = i % 4 == 2
            rate = (35, 45) if name == "angular_rates" else (10, 14)
            yaw[:, spin] = rng.uniform(-3, 3, spin.sum()) + np.where(rng.random(spin.sum()) < 0.5, -1, 1) * rng.uniform(*rate, spin.sum()) * t
            # angular rates: |sin pitch| >= cos(6e-3) > 0.9999, the gimbal branches (roll = 0, yaw = 2 atan2(qz, qw)); angular
            # velocities: 5e-2 short of them (the model's 1 / cos(pitch) at +-pi/2 exactly is not finite, in the reference too)
            gimbal = i % 8 == 3
            sign = np.where(i[gimbal] % 16 == 3, 1.0, -1.0)
            near = 4e-3 if name == "angular_rates" else 5e-2
            pitch[:, gimbal] = sign * (np.pi / 2 - near + 2e-3 * np.sin(3.0 * t))
            q = _quat(roll, pitch, yaw)
            p0[:, 3:] = q[0]
            meas[:, :, 3:] = q[1:]
        rng = np.random.default_rng(seed + 2)
        has = np.ones((T, NMAX), dtype=np.uint8)
        for s in range(T):
            if 150 <= s < 200 or s % 10 == 7:
                has[s] = 0
            elif s % 10 == 3:
                has[s] = rng.random(NMAX) < 0.7
        ns = oracle.MODEL_DIMS[oracle.MODELS[name]][0]
        v0 = rng.uniform(-0.5, 0.5, (NMAX, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
        a0 = rng.uniform(-0.5, 0.5, (NMAX, 6)) * 0.1
        scale = np.exp(rng.uniform(-0.7, 0.7, (NMAX, ns)))
        _cache[("stream", name)] = dict(p0=p0, meas=meas, has=has, v0=v0, a0=a0, scale=scale)
    return _cache[("stream", name)]


def edge_inputs(models, name, dtype, n, p0_per_target=True, coupled_matrices=False):
    """Everything a path and its oracles need, rounded to the precision of `dtype` (f32: every value an f32)."""
    m = models[name]
    st = _edge_stream(name)
    mats = coupled(m) if coupled_matrices else dict(Q=m["Q"], R=m["R"], P=m["P"])
    P0 = mats["P"]
    if p0_per_target:                      # D P0 D with a positive diagonal D per target: the structure of P0 stays
        s = st["scale"][:n]
        P0 = s[:, :, None] * P0[None] * s[:, None, :]
        P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))     # symmetric to the bit, as the layouts that store a triangle need
    rd = f32r if dtype == "f32" else (lambda a: np.array(a, dtype=np.float64))
    has = st["has"][:, :n]
    return dict(name=name, dtype=dtype, n=n, model=m["model"], Q=rd(mats["Q"]), R=rd(mats["R"]), P0=rd(P0), p0=rd(st["p0"][:n]),
                v0=rd(st["v0"][:n]), a0=rd(st["a0"][:n]), meas=rd(st["meas"][:, :n]), has=has,
                key=(name, dtype, n, p0_per_target, coupled_matrices))


def tick_mask(inp, s):
    """None (every target measured), "predict" (nobody) or the uint8 mask of tick s."""
    h = inp["has"][s]
    return None if h.all() else ("predict" if not h.any() else h)


def run_oracles(inp):
    """The same-precision oracle and the f80 oracle over the whole schedule (cached per input set): states after CHECK ticks,
    derived outputs (own time and t1) and the sphere query after the last tick."""
    if inp["key"] in _cache:
        return _cache[inp["key"]]
    res = {}
    for d in (inp["dtype"], "f80"):
        orc = oracle.OracleBatch(inp["model"], inp["Q"], inp["R"], inp["P0"], inp["p0"], DT, 0.0, inp["v0"], inp["a0"], dtype=d)
        st = {}
        for s in range(T):
            k = tick_mask(inp, s)
            orc.step(DT, None if isinstance(k, str) else inp["meas"][s], None if k is None or isinstance(k, str) else k, nthreads=THREADS)
            if s + 1 in CHECK:
                st[s + 1] = orc.state()
        t1 = T * DT + 0.1
        out = dict(now=np.concatenate([orc.pose(), orc.twist(), orc.acceleration()], 1),
                   at=np.concatenate([orc.pose_at(t1), orc.twist_at(t1), orc.acceleration_at(t1)], 1))
        ok, pose, delta = orc.intersection_pose(T * DT, ORIGIN, RADIUS)
        res[d] = dict(state=st, out=out, ix=(delta, pose), orc=orc)
    res["margin"] = _ix_margin(res["f80"]["orc"], T * DT)
    for d in (inp["dtype"], "f80"):
        del res[d]["orc"]
    _cache[inp["key"]] = res
    return res


def _ix_margin(orc, t1):
    """Distance of every target's sphere query from a classification boundary, from the f80 oracle's getters: |imag| of the
    complex roots, |value| of the smallest real one, gap between real roots (as ix_margin of tests/golden/make_highprec_kat.py)."""
    p, v, a = orc.pose_at(t1)[:, :3] - ORIGIN, orc.twist_at(t1)[:, :3], orc.acceleration_at(t1)[:, :3]
    margin = np.ones(orc.N)
    for i in range(orc.N):
        c = [(p[i] * p[i]).sum() - RADIUS ** 2, 2 * (p[i] * v[i]).sum(), (v[i] * v[i]).sum() + (p[i] * a[i]).sum(), (v[i] * a[i]).sum(),
             0.25 * (a[i] * a[i]).sum()]
        if c[4] == 0:
            continue
        r = oracle.poly_roots(c)
        mg = min([abs(z.imag) for z in r if abs(z.imag) >= 1e-10] + [1.0])
        real = sorted(z.real for z in r if abs(z.imag) < 1e-10)
        if real:
            mg = min([mg, abs(real[0])] + [real[j + 1] - real[j] for j in range(len(real) - 1)])
        margin[i] = mg
    return margin


def _row(tag, dtype, what, got, same, ref, ceiling, k=K):
    e_k = x_err(got, ref) if what != "P" else P_err(got, ref)
    e_o = x_err(same, ref) if what != "P" else P_err(same, ref)
    floor = 8 * EPS[dtype]
    e_s = x_err(got, same) if what != "P" else P_err(got, same)
    print("[precision] %-52s %-3s %-3s kernel %.2e  faithful %.2e  ratio %6.2f  (kernel vs %s oracle %.2e)"
          % (tag, dtype, what, e_k, e_o, e_k / max(e_o, floor), dtype, e_s))
    assert np.isfinite(got).all(), (tag, what)
    assert e_k <= k * e_o + floor, "%s %s: kernel error %.3e > %g x faithful %.3e + %.1e" % (tag, what, e_k, k, e_o, floor)
    assert e_k <= ceiling, "%s %s: kernel error %.3e over the ceiling %.1e" % (tag, what, e_k, ceiling)
    if what == "P":   # exact zeros of the f80 answer stay exact zeros
        assert np.all(got[ref == 0] == 0), (tag, "a structural zero of P is not zero")


def check_states(tag, inp, ref, tick, x, P):
    d, c = inp["dtype"], CEIL[inp["dtype"]][inp["name"]]
    xs, Ps = ref[d]["state"][tick]
    xr, Pr = ref["f80"]["state"][tick]
    _row("%s tick %d" % (tag, tick), d, "x", x, xs, xr, c["x"])
    _row("%s tick %d" % (tag, tick), d, "P", P, Ps, Pr, c["P"])


def _unsign(q, ref):
    """q or -q, whichever is nearer ref (the same rotation)"""
    flip = (np.abs(q - ref).max(1) > np.abs(q + ref).max(1))[:, None]
    return np.where(flip, -q, q)


def check_outputs(tag, inp, ref, now, at):
    d, c = inp["dtype"], CEIL[inp["dtype"]][inp["name"]]
    for which, got in (("now", now), ("at t1", at)):
        r, s = ref["f80"]["out"]["now" if which == "now" else "at"], ref[d]["out"]["now" if which == "now" else "at"].copy()
        got = got.copy()
        got[:, 3:7] = _unsign(got[:, 3:7], r[:, 3:7])
        s[:, 3:7] = _unsign(s[:, 3:7], r[:, 3:7])
        _row("%s outputs %s" % (tag, which), d, "out", got, s, r, c["out"])


def check_query(tag, inp, ref, delta, pose, min_hits=3):
    """delta and the pose at the intersection; hit / miss exactly where the f80 classification is clear."""
    d, c = inp["dtype"], CEIL[inp["dtype"]][inp["name"]]
    dr, pr = ref["f80"]["ix"]
    ds, ps = ref[d]["ix"]
    clear = ref["margin"] > 1e-3
    hit = dr > -1
    assert ((delta > -1) == hit)[clear].all(), (tag, np.nonzero(((delta > -1) != hit) & clear)[0])
    use = clear & hit & (ds > -1)
    assert use.sum() >= min_hits, (tag, "too few clear hits to measure", int(use.sum()))
    if not use.any():
        return
    got = np.concatenate([delta[use, None], pose[use, :3]], 1)
    _row("%s sphere query (%d hits)" % (tag, use.sum()), d, "ix", got, np.concatenate([ds[use, None], ps[use, :3]], 1),
         np.concatenate([dr[use, None], pr[use, :3]], 1), c["ix"])


def _manager(inp, lanes=0):
    mgr = te.TargetManager(dtype=inp["dtype"], lanes_per_target=lanes)
    ids = np.arange(inp["n"], dtype=np.uint32) * 5 + 2
    assert mgr.init_batch(ids, DT, 0.0, inp["p0"], inp["v0"], inp["a0"], type=inp["model"], Q=inp["Q"], R=inp["R"], P0=inp["P0"]) == inp["n"]
    return mgr, ids


def _dev(inp, b):
    meas = torch.from_numpy(np.ascontiguousarray(inp["meas"].transpose(0, 2, 1))).to("cuda").to(b.torch_dtype()).contiguous()
    has = torch.from_numpy(np.ascontiguousarray(inp["has"])).to("cuda")
    return meas, has


def _step_ticks(b, inp, meas, has, s0, s1):
    for s in range(s0, s1):
        k = tick_mask(inp, s)
        b.step(DT, None if isinstance(k, str) else meas[s], None if k is None or isinstance(k, str) else has[s])


def _outputs(mgr, ids):
    p, tw, ac, found = mgr.get_est_batch(ids)
    assert found.all()
    p1, tw1, ac1, found = mgr.get_est_batch(ids, t1=T * DT + 0.1)
    assert found.all()
    return np.concatenate([p, tw, ac], 1), np.concatenate([p1, tw1, ac1], 1)


# ---- per-batch kernels: every layout of LANES, tick by tick (b.step), masked and predict-only ticks --------------------------------
@pytest.mark.parametrize("name,dtype", [(m, d) for m in HARNESS_ORDER for d in ("f64", "f32")])
def test_per_batch_kernels(models, name, dtype):
    inp = edge_inputs(models, name, dtype, 333)
    ref = run_oracles(inp)
    for lanes in LANES[name][dtype]:
        mgr, ids = _manager(inp, lanes)
        b = mgr.batches()[0]
        meas, has = _dev(inp, b)
        tag = "%s lanes %d (%s)" % (name, lanes, b.layout)
        done = 0
        for c in CHECK:
            _step_ticks(b, inp, meas, has, done, c)
            done = c
            check_states(tag, inp, ref, c, *mgr.get_state_batch(ids))
        check_outputs(tag, inp, ref, *_outputs(mgr, ids))
        mgr.close()


# ---- the dense kernel: Q, R, P0 that couple every axis (symmetric-packed P) -------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [(m, d) for m in HARNESS_ORDER for d in ("f64", "f32")])
def test_coupled_matrices_dense_kernel(models, name, dtype):
    inp = edge_inputs(models, name, dtype, 333, coupled_matrices=True)
    ref = run_oracles(inp)
    mgr, ids = _manager(inp)
    b = mgr.batches()[0]
    assert b.layout == "symmetric_packed"
    meas, has = _dev(inp, b)
    done = 0
    for c in CHECK:
        _step_ticks(b, inp, meas, has, done, c)
        done = c
        check_states("%s coupled (dense)" % name, inp, ref, c, *mgr.get_state_batch(ids))
    check_outputs("%s coupled (dense)" % name, inp, ref, *_outputs(mgr, ids))
    mgr.close()


# ---- graph replay: step_sequence(use_graph=True), the automatic layout, 65 targets ---------------------------------------------------
@pytest.mark.parametrize("name,dtype", [(m, d) for m in HARNESS_ORDER for d in ("f64", "f32")])
def test_graph_replay(models, name, dtype):
    inp = edge_inputs(models, name, dtype, 65)
    ref = run_oracles(inp)
    mgr, ids = _manager(inp, LANES[name][dtype][0])
    b = mgr.batches()[0]
    meas, has = _dev(inp, b)
    done = 0
    for c in CHECK:
        b.step_sequence(DT, meas[done:c], has[done:c], use_graph=True)
        done = c
        check_states("%s graph replay" % name, inp, ref, c, *mgr.get_state_batch(ids))
    mgr.close()


# ---- the population kernel (one launch per tick for every batch) with the fused sphere query ---------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_population_kernel_and_fused_query(models, dtype):
    sizes = {"angular_rates": 333, "angular_velocities": 65, "uniform_acceleration": 63, "uniform_velocity": 1}
    inps = [edge_inputs(models, name, dtype, n, p0_per_target=False) for name, n in sizes.items()]
    refs = [run_oracles(inp) for inp in inps]
    mgr = te.TargetManager(dtype=dtype)
    base, idss = 0, []
    for inp in inps:
        ids = np.arange(inp["n"], dtype=np.uint32) + base
        base += inp["n"]
        assert mgr.init_batch(ids, DT, 0.0, inp["p0"], inp["v0"], inp["a0"], type=inp["model"], Q=inp["Q"], R=inp["R"], P0=inp["P0"]) == inp["n"]
        idss.append(ids)
    assert mgr.population_tick()
    bs = mgr.batches()
    dev = [_dev(inp, b) for inp, b in zip(inps, bs)]
    deltas = [torch.full((b.size,), 123.0, dtype=torch.float64, device="cuda") for b in bs]
    poses = [torch.zeros((b.size, 7), dtype=torch.float64, device="cuda") for b in bs]
    done = 0
    for c in CHECK:
        mgr.step_sequence_all(DT, [m[done:c] for m, _ in dev], has_meas=[h[done:c] for _, h in dev], use_graph=0,
                              query=(ORIGIN, RADIUS, deltas, poses))
        done = c
        for inp, ref, ids in zip(inps, refs, idss):
            check_states("%s population (%d)" % (inp["name"], inp["n"]), inp, ref, c, *mgr.get_state_batch(ids))
    torch.cuda.synchronize()
    for inp, ref, d, p in zip(inps, refs, deltas, poses):
        if inp["name"] in ("uniform_acceleration", "angular_rates"):       # the models with an acceleration: a quartic to solve
            check_query("%s population fused query" % inp["name"], inp, ref, d.cpu().numpy(), p.cpu().numpy(),
                        min_hits=3 if inp["name"] == "angular_rates" else 0)
    mgr.close()


# ---- the resident ("live") kernel: sessions continuing through the ring, compared after every live_stop ----------------------------
@pytest.mark.parametrize("name,dtype", [(m, d) for m in HARNESS_ORDER for d in ("f64", "f32")])
def test_resident_kernel(models, name, dtype):
    inp = edge_inputs(models, name, dtype, 63)
    ref = run_oracles(inp)
    live = torch.cuda.Stream()              # the session's manager on its own non-blocking stream (as tests/test_gpu_live.py)
    mgr, ids = _manager(inp)
    mgr.set_stream(live.cuda_stream)
    mgr.synchronize()
    b = mgr.batches()[0]
    meas, has = _dev(inp, b)
    torch.cuda.synchronize()
    done = 0
    for c in CHECK:
        b.live_start(DT, meas, has, first_entry=done, max_ticks=c - done, idle_limit_s=3.0)
        b.live_post(c - done)
        assert b.live_wait(c - done, 10.0)
        assert b.live_stop() == c - done
        done = c
        check_states("%s resident" % name, inp, ref, c, *mgr.get_state_batch(ids))
    mgr.close()


# ---- the one-target queue (by-id calls of at most kSmallBatchQueue = 1024 targets) and the bulk path just past it ------------------
@pytest.mark.parametrize("name,dtype,n", [("uniform_acceleration", "f64", k) for k in (1, 40, 300, 1024, 1025)]
                         + [(m, d, 300) for m in HARNESS_ORDER for d in ("f64", "f32") if (m, d) != ("uniform_acceleration", "f64")]
                         + [("angular_rates", "f32", 1025)])
def test_by_id_calls(models, name, dtype, n):
    inp = edge_inputs(models, name, dtype, n)
    ref = run_oracles(inp)
    mgr, ids = _manager(inp)
    perm = np.random.default_rng(n).permutation(n)
    done = 0
    for c in CHECK:
        for s in range(done, c):
            k = tick_mask(inp, s)
            if isinstance(k, str):
                mgr.update_batch(ids[perm], DT, inp["meas"][s][perm], np.zeros(n, dtype=np.uint8))
            else:
                mgr.update_batch(ids[perm], DT, inp["meas"][s][perm], None if k is None else k[perm])
        done = c
        check_states("%s by id (%d)" % (name, n), inp, ref, c, *mgr.get_state_batch(ids))
    check_outputs("%s by id (%d)" % (name, n), inp, ref, *_outputs(mgr, ids))
    if name in ("uniform_acceleration", "angular_rates"):     # the models with an acceleration: a quartic to solve
        delta, pose, found = mgr.intersect_batch(ids, T * DT, ORIGIN, RADIUS)
        assert found.all()
        check_query("%s intersect_batch (%d)" % (name, n), inp, ref, delta, pose, min_hits=3 if name == "angular_rates" and n >= 300 else 0)
    mgr.close()
