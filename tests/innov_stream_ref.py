"""Reference and bounds for the per-tick innovation stream (tests/test_gpu_innov_stream.py, tests/test_innov_stream_abi.py).

The reference of every numeric check is oracle/np_twin.py's Target, one per target: before each add_measurement the innovation
nu = y - x^-[0:m], S = P^-[0:m,0:m] + R, w = S^-1 nu and NIS = nu^T w are formed from the twin's own x, P and meas_rpy.

The bounds come from TOL[dtype] of tests/test_gpu_parity.py, the tolerance every kernel path is already held to on x and P;
no new constant.  With e_c = x_atol + x_rtol |x^-_c| the innovation may differ by |d nu_c| <= e_c (y is exact, x^- is a state
within the state tolerance), and to first order plus the quadratic remainder
    |d NIS| <= 2 |w|^T e + e^T |S^-1| e + P_rel max|P^-| (sum_c |w_c|)^2,
the last term being w^T dS w with every |dS_ij| <= P_rel max|P^-| (the tolerance on P, relative to the matrix's largest entry).
This bound is coarse (a tenth of the NIS in fp32); tests/test_gpu_precision_streams.py holds nu and the NIS of every path to the
extended-precision oracle within 8 x the same-precision oracle's own error, on harder inputs."""
import functools

import numpy as np

from oracle import np_twin as tw
from test_gpu_parity import TOL

PREDICT_ONLY = range(11, 15)    # a run of ticks on which no target has a measurement


def masks(ticks, N, seed):
    """Bernoulli(0.9) masks [ticks, N] uint8 with a predict-only run"""
    rng = np.random.default_rng(seed + 1)
    mask = (rng.random((ticks, N)) < 0.9).astype(np.uint8)
    for s in PREDICT_ONLY:
        if s < ticks:
            mask[s] = 0
    return mask


def twin_innovations(model, Q, R, P0, p0, meas, mask, dt):
    """One np_twin.Target per target over the stream.  Returns a dict of [ticks, N, ...] arrays: nu, nis (0 / -1 where the target
    has no measurement), and what the bounds need -- xm = x^-[0:m], w = S^-1 nu, Sinv, pmax = max|P^-| -- plus the final x, P."""
    ticks, N = meas.shape[0], meas.shape[1]
    n, m = tw.DIMS[model]
    out = dict(nu=np.zeros((ticks, N, m)), nis=np.full((ticks, N), -1.0), xm=np.zeros((ticks, N, m)), w=np.zeros((ticks, N, m)),
               Sinv=np.zeros((ticks, N, m, m)), pmax=np.zeros((ticks, N)), x=np.zeros((N, n)), P=np.zeros((N, n, n)))
    for j in range(N):
        t = tw.Target(model, Q, R, P0, p0[j], dt)
        for s in range(ticks):
            if not mask[s, j]:
                t.update(dt)
                continue
            A = t._A(dt)
            xm = t._f(t.x, dt) if model == tw.ANGULAR_VELOCITIES else A @ t.x
            Pm = A @ t.P @ A.T + t.Q
            y = meas[s, j, 0:3].copy()
            if m == 6:
                y = np.concatenate([y, tw.unwrap(t.meas_rpy, tw.quat_to_rpy(tw.quat_normalize(meas[s, j, 3:7])))])
            nu = y - xm[:m]
            Sinv = np.linalg.inv(Pm[:m, :m] + t.R)
            w = Sinv @ nu
            out["nu"][s, j], out["nis"][s, j], out["xm"][s, j], out["w"][s, j] = nu, nu @ w, xm[:m], w
            out["Sinv"][s, j], out["pmax"][s, j] = Sinv, np.abs(Pm).max()
            t.add_measurement(dt, meas[s, j])
        out["x"][j], out["P"][j] = t.x, t.P
    return out


@functools.lru_cache(maxsize=None)
def _cached(name, N, ticks, seed):
    import oracle
    from conftest import model_path, synth_stream
    m = oracle.load_model_yaml(model_path(name))
    p0, meas = synth_stream(name, N, ticks, seed=seed)
    mask = masks(ticks, N, seed)
    ref = twin_innovations(m["model"], m["Q"], m["R"], m["P"], p0, meas, mask, 0.004)
    for v in (p0, meas, mask, *ref.values()):
        v.setflags(write=False)   # shared among the tests: nobody changes it
    return p0, meas, mask, ref


def stream_and_reference(name, N, ticks, seed):
    """p0 [N,7], meas [ticks,N,7], mask [ticks,N] and the twin's innovations for the shipped model `name` at dt = 0.004: computed
    once per (name, N, ticks, seed) and shared, read-only."""
    return _cached(name, N, ticks, seed)


def bounds(ref, dtype):
    """(e [ticks,N,m], nis_bound [ticks,N]) of the module docstring for TOL[dtype]"""
    t = TOL[dtype]
    e = t["x_atol"] + t["x_rtol"] * np.abs(ref["xm"])
    aw = np.abs(ref["w"])
    quad = np.einsum("snr,snrc,snc->sn", e, np.abs(ref["Sinv"]), e)
    return e, 2.0 * (aw * e).sum(-1) + quad + t["P_rel"] * ref["pmax"] * aw.sum(-1) ** 2


def check(nu, nis, ref, mask, dtype, what=""):
    """nu [ticks,N,m] (or None), nis [ticks,N] against the twin: the sentinels exactly where the mask is 0, every other target of
    every tick within the bounds.  Prints the worst ratios before it asserts."""
    has = mask.astype(bool)
    e, nb = bounds(ref, dtype)
    assert (nis[~has] == -1.0).all(), "%s: NIS of a target without a measurement is not -1" % what
    assert (nis[has] >= 0.0).all(), "%s: a measured target has a negative NIS" % what
    r_nis = (np.abs(nis - ref["nis"])[has] / nb[has]).max() if has.any() else 0.0
    r_nu = 0.0
    if nu is not None:
        assert (nu[~has] == 0.0).all(), "%s: innovation of a target without a measurement is not 0" % what
        r_nu = (np.abs(nu - ref["nu"])[has] / e[has]).max() if has.any() else 0.0
    print("%s: worst |d nu| / bound %.3g, worst |d NIS| / bound %.3g" % (what, r_nu, r_nis))
    assert r_nu <= 1.0, "%s: an innovation is %.3g times its bound away from the twin" % (what, r_nu)
    assert r_nis <= 1.0, "%s: a NIS is %.3g times its bound away from the twin" % (what, r_nis)


def oracle_innovations(model, Q, R, P0, p0, meas, mask, dt, dtype):
    """An independent implementation at the precision `dtype`: oracle.OracleBatch stepped over the stream, nu / NIS formed in numpy
    (arrays of that precision) from its state() before each tick, with an unwrap memory kept by the reference's rule."""
    import oracle
    ft = np.float64 if dtype == "f64" else np.float32
    ticks, N = meas.shape[0], meas.shape[1]
    n, m = tw.DIMS[model]
    orc = oracle.OracleBatch(model, Q, R, P0, p0, dt, dtype=dtype)
    Qt, Rt = np.asarray(Q, ft), np.asarray(R, ft)
    nu_o, nis_o = np.zeros((ticks, N, m)), np.full((ticks, N), -1.0)
    rpy_mem = np.zeros((N, 3), ft)
    probe = tw.Target(model, Q, R, P0, p0[0], dt)   # (for _A / _f on a given x)
    for s in range(ticks):
        x, P = orc.state()
        for j in range(N):
            if not mask[s, j]:
                continue
            xj, Pj = x[j].astype(ft), P[j].astype(ft)
            probe.x = xj.astype(float)
            A = probe._A(dt).astype(ft)
            xm = probe._f(xj.astype(float), dt).astype(ft) if model == tw.ANGULAR_VELOCITIES else A @ xj
            S = (A @ Pj @ A.T + Qt)[:m, :m] + Rt
            y = meas[s, j, 0:3].astype(ft)
            if m == 6:
                rpy = tw.unwrap(rpy_mem[j].astype(float), tw.quat_to_rpy(tw.quat_normalize(meas[s, j, 3:7].astype(ft).astype(float)))).astype(ft)
                rpy_mem[j] = rpy
                y = np.concatenate([y, rpy])
            nu = (y - xm[:m]).astype(ft)
            w = (np.linalg.inv(S).astype(ft) @ nu).astype(ft)
            nu_o[s, j], nis_o[s, j] = nu, ft(nu @ w)
        orc.step(dt, meas[s], mask[s])
    return nu_o, nis_o
