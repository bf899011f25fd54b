"""Reference and stream for the re-acquisition of lost tracks inside the gated ticks (tests/test_reacquire_reference.py,
tests/test_gpu_reacquire.py), on top of tests/gate_ref.py.

stream(name) is gate_ref.stream(name) plus the jump: +0.5 m on x from tick JUMP_TICK on, for 24 targets drawn with default_rng(7).
twin_reacquire is gate_ref.twin_gated with the run of consecutive rejections per target; on a re-initialisation it builds a fresh
np_twin.Target from that tick's measurement with the same Q, R, P0.  event_rule is the rule alone, for host counters kept from
NIS rows read back."""
import functools

import numpy as np

import gate_ref
from oracle import np_twin as tw

N, TICKS, DT = gate_ref.N, gate_ref.TICKS, gate_ref.DT
JUMP_TICK, JUMP = 8, 0.5
JUMPED = np.sort(np.random.default_rng(7).choice(N, 24, replace=False))
JUMPED.setflags(write=False)


@functools.lru_cache(maxsize=None)
def stream(name):
    """p0, meas (with gate_ref's outliers and the jump), mask, outlier, spikes -- read-only, shared"""
    p0, meas, mask, outlier, spikes = gate_ref.stream(name)
    meas = meas.copy()
    meas[JUMP_TICK:, JUMPED, 0] += JUMP
    meas.setflags(write=False)
    return p0, meas, mask, outlier, spikes


def event_rule(c, measured, accepted, can_init, K):
    """one slot, one tick: (stored run, event byte, re-initialised) from the run c before the tick"""
    if not measured:
        return c, 0, False
    if accepted:
        return 0, 0, False
    c1 = min(c + 1, 127)
    if K > 0 and c1 >= K and can_init:
        return 0, 0x80 | c1, True
    return c1, c1, False


def initial_state_is_finite(model, y):
    """is the initial state that a fresh target forms from the measurement y [7] finite in every component?"""
    with np.errstate(all="ignore"):
        if model in (tw.ANGULAR_RATES, tw.ANGULAR_VELOCITIES):
            return bool(np.isfinite(y[0:3]).all() and np.isfinite(tw.quat_to_rpy(tw.quat_normalize(y[3:7]))).all())
        return bool(np.isfinite(y[0:3]).all())


def twin_reacquire(model, Q, R, P0, p0, meas, mask, dt, gamma, K):
    """gate_ref.twin_gated with the run counter: the same dict plus run [N] (at the end) and event [ticks, N] uint8"""
    ticks, n_t = meas.shape[0], meas.shape[1]
    n, m = tw.DIMS[model]
    out = dict(nu=np.zeros((ticks, n_t, m)), nis=np.full((ticks, n_t), -1.0), xm=np.zeros((ticks, n_t, m)), w=np.zeros((ticks, n_t, m)),
               Sinv=np.zeros((ticks, n_t, m, m)), pmax=np.zeros((ticks, n_t)), x=np.zeros((n_t, n)), P=np.zeros((n_t, n, n)),
               acc=np.zeros((ticks, n_t), bool), run=np.zeros(n_t, np.uint8), event=np.zeros((ticks, n_t), np.uint8))
    for j in range(n_t):
        t = tw.Target(model, Q, R, P0, p0[j], dt)
        c = 0
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
            nis = nu @ w
            out["nu"][s, j], out["nis"][s, j], out["xm"][s, j], out["w"][s, j] = nu, nis, xm[:m], w
            out["Sinv"][s, j], out["pmax"][s, j] = Sinv, np.abs(Pm).max()
            accepted = bool(nis <= gamma)     # (a NaN rejects)
            c, ev, init = event_rule(c, True, accepted, initial_state_is_finite(model, meas[s, j]), K)
            out["event"][s, j] = ev
            if accepted:
                out["acc"][s, j] = True
                t.add_measurement(dt, meas[s, j])
            elif init:
                t = tw.Target(model, Q, R, P0, meas[s, j], dt)
            else:
                t.update(dt)
        out["x"][j], out["P"][j], out["run"][j] = t.x, t.P, c
    return out


@functools.lru_cache(maxsize=None)
def reference(name, gamma, K):
    """the twin over stream(name) at (gamma, K), computed once and shared, read-only"""
    import oracle
    from conftest import model_path
    mdl = oracle.load_model_yaml(model_path(name))
    p0, meas, mask, _, _ = stream(name)
    out = twin_reacquire(mdl["model"], mdl["Q"], mdl["R"], mdl["P"], p0, meas, mask, DT, gamma, K)
    for v in out.values():
        v.setflags(write=False)
    return out
