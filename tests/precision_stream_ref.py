"""The reference side of the stream rows of the precision matrix (tests/test_gpu_precision_streams.py on the GPU,
tests/test_oracle_innovations.py for the conditions it rests on, on the CPU).

Inputs are edge_inputs of tests/test_gpu_precision.py.  Two CPU oracles take the schedule, the strict oracle in the kernel's
precision and the f80 oracle, and before every step OracleBatch.innovations gives the nu = y - C x^- and NIS = nu^T S^-1 nu that
step forms -- in the oracle's precision, the unwrap taken against its own memory.  With acc= both are stepped with that accept
mask in place of the schedule's own (innovations still asked with the schedule's mask), which is how a gated kernel's trajectory
is followed.

Metric, per input group and window (the maxima over the measured pairs of the group in the window):
    e_nu  = |d nu|_inf / max(1, |C x^-|_inf)     C x^- of the f80 run: x_err of test_highprec_kat.py on the quantity subtracted
    e_nis = |d NIS| / max(1, NIS_f80)
Groups (by target index i; judged apart, because a faithful fp32 NIS on the far group is off by 0.3 to 1.0 relative -- an f32
near 1.2e4 m has a 1 mm ulp against the 1 cm sigma -- while the other groups are faithful to about 1e-3): far i % 4 == 1, spin
i % 4 == 2, gimbal i % 8 == 3, plain the rest.  Windows: the five between the CHECK ticks, (0,1] (1,10] (10,100] (100,200]
(200,300]."""
import numpy as np

import oracle
from test_gpu_precision import CHECK, DT, EPS, K, T, THREADS, edge_inputs, tick_mask

GROUPS = ("far", "spin", "gimbal", "plain")
WINDOWS = tuple(zip((0,) + CHECK[:-1], CHECK))      # (lo, hi]: ticks lo .. hi - 1 counted from 0

# ---- the gate of the decision rows: chosen on the CPU from the f80 oracle gating itself over stream_inputs(name, dtype, 333) (step
# with has & (nis <= gamma), nis from its own innovations) so that between 5 % and 60 % of the measured pairs of the groups judged
# (all four in fp64, the far group left out in fp32) are rejected; tests/test_oracle_innovations.py asserts it.  The chi-square
# 0.99 quantile does it for uniform velocity and angular rates (a rejected target drifts and is rejected again, so the shares are
# far above 1 %).  Uniform acceleration starts with per-target v0, a0 under a measured motion that carries gravity: its NIS has a
# median near 150, the quantile would reject 91 %, and its gate is 1000.  Angular velocities: at the quantile (16.812) the targets
# of the gimbal group, once rejected, are lost for good, and an EKF coasting 5e-2 rad from pitch = pi/2 is no reference -- max|P|
# reaches 1e7, the f64 oracle's P is 9e-7 from the f80 oracle's and the f32 oracle's NIS is not finite on three pairs -- so its gate
# is 30, where the gimbal group still meets rejections (0.2 % of its pairs; spin 92 %) and recovers, and both oracles stay within
# the ceilings of tests/test_gpu_precision.py.  REJECTED: the f80 reference's shares, fp64 inputs / fp32 inputs.
GAMMA = {"uniform_velocity": 11.345, "uniform_acceleration": 1000.0, "angular_rates": 16.812, "angular_velocities": 30.0}
REJECTED = {"uniform_velocity": (0.520, 0.515), "uniform_acceleration": (0.400, 0.400), "angular_rates": (0.422, 0.475),
            "angular_velocities": (0.261, 0.329)}
_cache = {}


# fp64 only: the far group's offset as a fraction of edge_inputs' (1.2e4, -0.7e4, 0.4e4) m.  At the full offset the f64 oracle's NIS
# on that group is 8e-10 to 7e-9 from the f80 oracle's (an f64 near 1.2e4 m has a 2e-12 m ulp against the 1 cm sigma, and
# w = S^-1 nu is of order 1e3), over the 1e-10 a stream row's reference must stay under to mean something
# (tests/test_oracle_innovations.py); the error is linear in the offset, and at 1 / 256 of it (47, -27, 16 m, still five times
# synth_stream's own 10 m) it is 3e-11.  fp32 keeps the full offset: its far group is judged apart.
FAR_FRACTION_F64 = 1.0 / 256.0
FAR_OFFSET = np.array([1.2e4, -0.7e4, 0.4e4])


def stream_inputs(models, name, dtype, n, **kw):
    """edge_inputs for the stream rows: the same, with the fp64 far group moved in (FAR_FRACTION_F64)"""
    inp = edge_inputs(models, name, dtype, n, **kw)
    if dtype == "f64":
        inp = dict(inp)
        far = np.arange(n) % 4 == 1
        back = FAR_OFFSET * (1.0 - FAR_FRACTION_F64)
        inp["p0"], inp["meas"] = inp["p0"].copy(), inp["meas"].copy()
        inp["p0"][far, :3] -= back
        inp["meas"][:, far, :3] -= back
        inp["key"] = inp["key"] + ("far / 256",)
    return inp


def group_of(n):
    """[n] array of indices into GROUPS"""
    i = np.arange(n)
    g = np.full(n, GROUPS.index("plain"))
    g[i % 4 == 1] = GROUPS.index("far")
    g[i % 4 == 2] = GROUPS.index("spin")
    g[i % 8 == 3] = GROUPS.index("gimbal")
    return g


def judged_groups(dtype):
    """the groups a decision test judges: the fp32 far group's faithful error spans any gate"""
    return tuple(g for g in GROUPS if not (dtype == "f32" and g == "far"))


def window_of():
    """[T] window index of every tick"""
    w = np.zeros(T, dtype=int)
    for k, (lo, hi) in enumerate(WINDOWS):
        w[lo:hi] = k
    return w


def run_stream_oracles(inp, acc=None, key=None):
    """{dtype, "f80"} -> dict(nu [T,N,m], nis [T,N], hx [T,N,m], state {tick: (x, P)}) over the schedule of inp, stepped with
    the schedule's masks or with acc [T,N]; cached per input set (and `key` for an acc)."""
    ck = ("streams", inp["key"], key)
    if acc is None or key is not None:
        if ck in _cache:
            return _cache[ck]
    has = inp["has"].astype(np.uint8)
    res = {}
    for d in (inp["dtype"], "f80"):
        orc = oracle.OracleBatch(inp["model"], inp["Q"], inp["R"], inp["P0"], inp["p0"], DT, 0.0, inp["v0"], inp["a0"], dtype=d)
        nu, nis, hx, st = np.zeros((T, orc.N, orc.m)), np.full((T, orc.N), -1.0), np.zeros((T, orc.N, orc.m)), {}
        for s in range(T):
            if has[s].any():
                nu[s], nis[s], hx[s] = orc.innovations(DT, inp["meas"][s], has[s], nthreads=THREADS, with_pred=True)
            if acc is None:
                k = tick_mask(inp, s)
                orc.step(DT, None if isinstance(k, str) else inp["meas"][s], None if k is None or isinstance(k, str) else k, nthreads=THREADS)
            else:
                orc.step(DT, inp["meas"][s], np.ascontiguousarray(acc[s], dtype=np.uint8), nthreads=THREADS)
            if s + 1 in CHECK:
                st[s + 1] = orc.state()
        res[d] = dict(nu=nu, nis=nis, hx=hx, state=st)
    if acc is None or key is not None:
        _cache[ck] = res
    return res


def errors(nu, nis, ref80, has):
    """(e_nu, e_nis) [T, N] of the module docstring against the f80 run; 0 where the pair is not measured"""
    hasb = has.astype(bool)
    scale = np.maximum(1.0, np.abs(ref80["hx"]).max(-1))
    with np.errstate(invalid="ignore"):
        e_nu = np.where(hasb, np.abs(nu - ref80["nu"]).max(-1) / scale, 0.0)
        e_nis = np.where(hasb, np.abs(nis - ref80["nis"]) / np.maximum(1.0, ref80["nis"]), 0.0)
    return e_nu, e_nis


def rows(e, has):
    """[len(GROUPS), len(WINDOWS)] maxima of e [T,N] over the measured pairs of each group and window (NaN: none measured)"""
    hasb = has.astype(bool)
    g, w = group_of(e.shape[1]), window_of()
    out = np.full((len(GROUPS), len(WINDOWS)), np.nan)
    for a in range(len(GROUPS)):
        for b in range(len(WINDOWS)):
            sel = hasb[w == b][:, g == a]
            if sel.any():
                out[a, b] = e[w == b][:, g == a][sel].max()
    return out


def faithful(inp, ref=None):
    """(f_nu, f_nis) [groups, windows]: what the same-precision oracle errs by against the f80 oracle"""
    ref = run_stream_oracles(inp) if ref is None else ref
    e_nu, e_nis = errors(ref[inp["dtype"]]["nu"], ref[inp["dtype"]]["nis"], ref["f80"], inp["has"])
    return rows(e_nu, inp["has"]), rows(e_nis, inp["has"])


def self_gated(inp, gamma, dtype="f80"):
    """The oracle of `dtype` gating itself over the schedule: acc [T,N] bool = has & (nis <= gamma), nis [T,N] from its own
    innovations before every step, and the state after the last tick."""
    has = inp["has"].astype(np.uint8)
    orc = oracle.OracleBatch(inp["model"], inp["Q"], inp["R"], inp["P0"], inp["p0"], DT, 0.0, inp["v0"], inp["a0"], dtype=dtype)
    acc, nis = np.zeros((T, orc.N), bool), np.full((T, orc.N), -1.0)
    for s in range(T):
        if has[s].any():
            _, nis[s] = orc.innovations(DT, inp["meas"][s], has[s], nthreads=THREADS)
            acc[s] = has[s].astype(bool) & (nis[s] <= gamma)
        orc.step(DT, inp["meas"][s], acc[s].astype(np.uint8), nthreads=THREADS)
    return acc, nis


def rejected_share(acc, has, dtype):
    """share of the measured pairs of the judged groups that acc rejects"""
    g = group_of(acc.shape[1])
    cols = np.isin(g, [GROUPS.index(k) for k in judged_groups(dtype)])
    hasb = has.astype(bool)[:, cols]
    return float((hasb & ~acc[:, cols]).sum() / hasb.sum())


def decision_margin(inp, ref, f_nis):
    """[T,N]: how far NIS_f80 may be from the gate where a faithful kernel still decides differently:
    K e_faithful(group, window) max(1, NIS_f80) + 8 eps max(1, NIS_f80)"""
    g, w = group_of(inp["n"]), window_of()
    f = np.nan_to_num(f_nis)[g[None, :], w[:, None]]
    return (K * f + 8 * EPS[inp["dtype"]]) * np.maximum(1.0, ref["f80"]["nis"])


def judge_decisions(inp, acc, gamma, tag):
    """acc [T,N]: the accept mask of a gated run (a kernel's, from its own NIS rows).  Both oracles are run with has_meas = acc, so
    that all three sides follow one trajectory, innovations asked with the schedule's mask; a pair is `different` if acc differs
    from NIS_f80 <= gamma, `inside` if |NIS_f80 - gamma| <= decision_margin.  Returns dict(ref, f_nu, f_nis, unexplained = number of
    different pairs outside the margin, inside = share of the judged measured pairs inside it, different = their number)."""
    import hashlib
    ref = run_stream_oracles(inp, acc=acc, key=hashlib.sha1(np.ascontiguousarray(acc, dtype=np.uint8).tobytes()).hexdigest())
    f_nu, f_nis = faithful(inp, ref)
    mg = decision_margin(inp, ref, f_nis)
    cols = np.isin(group_of(inp["n"]), [GROUPS.index(k) for k in judged_groups(inp["dtype"])])
    has = inp["has"].astype(bool) & cols[None, :]
    inside = has & (np.abs(ref["f80"]["nis"] - gamma) <= mg)
    different = has & (acc.astype(bool) != (ref["f80"]["nis"] <= gamma))
    bad = different & ~inside
    out = dict(ref=ref, f_nu=f_nu, f_nis=f_nis, unexplained=int(bad.sum()), inside=float(inside.sum() / has.sum()),
               different=int(different.sum()), rejected=float((has & ~acc.astype(bool)).sum() / has.sum()))
    print("[decisions] %-46s gamma %-7g rejected %.3f  differ from the f80 decision %d (outside the margin %d)  inside the margin %.4f"
          % (tag, gamma, out["rejected"], out["different"], out["unexplained"], out["inside"]))
    for s, j in zip(*np.nonzero(bad)):
        print("    tick %d target %d: NIS_f80 %.9g, margin %.3g, accepted %d" % (s + 1, j, ref["f80"]["nis"][s, j], mg[s, j], acc[s, j]))
    return out


def row_failures(e_k, e_f, dtype):
    """the (group, window) rows of e_k [groups, windows] that break  e_kernel <= K e_faithful + 8 eps(dtype)"""
    with np.errstate(invalid="ignore"):
        return [(a, b) for a, b in zip(*np.nonzero(e_k > K * e_f + 8 * EPS[dtype]))]


def judge_rows(tag, inp, ref, nis, nu=None):
    """A path's stream, nis [T,N] and nu [T,N,m] (or None: a path that reports the NIS only), against the two oracle runs of ref:
    the sentinels exactly where the schedule's mask is 0 (the predict-only ticks included), every value of a measured pair
    finite, and per group, window and quantity  e_kernel <= K e_faithful + 8 eps(dtype).  Prints every row's ratio, then asserts.
    Returns the worst ratio e_kernel / max(e_faithful, 8 eps) over the judged rows (the fp32 far group included: its faithful
    error is large, its rule the same)."""
    d = inp["dtype"]
    has = inp["has"].astype(bool)
    assert nis.shape == has.shape
    assert (nis[~has] == -1.0).all(), "%s: the NIS of a target without a measurement is not -1" % tag
    assert np.isfinite(nis[has]).all(), "%s: a measured pair without a finite NIS" % tag
    if nu is not None:
        assert (nu[~has] == 0.0).all(), "%s: the innovation of a target without a measurement is not 0" % tag
        assert np.isfinite(nu[has]).all(), "%s: a measured pair without a finite innovation" % tag
    k_nu, k_nis = errors(ref["f80"]["nu"] if nu is None else nu, nis, ref["f80"], has)
    f_nu, f_nis = faithful(inp, ref)
    floor, worst, bad = 8 * EPS[d], 0.0, []
    for what, e_k, e_f in (("nu", rows(k_nu, has), f_nu), ("NIS", rows(k_nis, has), f_nis)):
        if what == "nu" and nu is None:
            continue
        for a, g in enumerate(GROUPS):
            ratio = e_k[a] / np.maximum(e_f[a], floor)
            print("[streams] %-50s %s %-6s %-3s kernel %s  faithful %s  ratio %s"
                  % (tag, d, g, what, " ".join("%.1e" % v for v in e_k[a]), " ".join("%.1e" % v for v in e_f[a]), " ".join("%5.2f" % v for v in ratio)))
            if not np.isnan(ratio).all():
                worst = max(worst, float(np.nanmax(ratio)))
        bad += ["%s %s window (%d,%d]: kernel %.3e > %g x faithful %.3e + %.1e" % (GROUPS[a], what, *WINDOWS[b], e_k[a, b], K, e_f[a, b], floor)
                for a, b in row_failures(e_k, e_f, d)]
    assert not bad, "%s: %s" % (tag, "; ".join(bad))
    return worst
