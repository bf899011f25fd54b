"""Schedule and reference for the calls with a time step per tick (tests/test_dt_schedule_reference.py, tests/test_gpu_dt_schedule*.py),
on top of tests/reacquire_ref.py.

The stream is reacquire_ref.stream(name): 203 targets, 20 ticks, masked ticks, outliers, the jump.  Its measurements were generated
for a constant DT; the schedule below is DT * f[s] with f drawn once over [0.25, 2], one tick at exactly 0.0 and one at 3 DT, so
the gate's decisions differ from those of the fixed-dt tests.  twin(name, gamma, K) is reacquire_ref.twin_reacquire with tick s
stepped at SCHEDULE[s] (gamma None: no gate, every measurement folded in)."""
import functools

import numpy as np

import reacquire_ref as rq
from oracle import np_twin as tw

N, TICKS, DT = rq.N, rq.TICKS, rq.DT
SEED = 11
ZERO_TICK, LONG_TICK = 5, 13


def make_schedule(seed=SEED, ticks=TICKS):
    dt = DT * np.random.default_rng(seed).uniform(0.25, 2.0, ticks)
    dt[ZERO_TICK % ticks] = 0.0
    dt[LONG_TICK % ticks] = 3.0 * DT
    return dt


SCHEDULE = make_schedule()
SCHEDULE.setflags(write=False)


def twin_schedule(model, Q, R, P0, p0, meas, mask, dts, gamma, K):
    """reacquire_ref.twin_reacquire with a dt per tick.  gamma None: ungated (K is ignored, no events)."""
    ticks, n_t = meas.shape[0], meas.shape[1]
    n, m = tw.DIMS[model]
    out = dict(nu=np.zeros((ticks, n_t, m)), nis=np.full((ticks, n_t), -1.0), xm=np.zeros((ticks, n_t, m)), w=np.zeros((ticks, n_t, m)),
               Sinv=np.zeros((ticks, n_t, m, m)), pmax=np.zeros((ticks, n_t)), x=np.zeros((n_t, n)), P=np.zeros((n_t, n, n)),
               acc=np.zeros((ticks, n_t), bool), run=np.zeros(n_t, np.uint8), event=np.zeros((ticks, n_t), np.uint8))
    for j in range(n_t):
        t = tw.Target(model, Q, R, P0, p0[j], DT)
        c = 0
        for s in range(ticks):
            dt = float(dts[s])
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
            if gamma is None:
                out["acc"][s, j] = True
                t.add_measurement(dt, meas[s, j])
                continue
            accepted = bool(nis <= gamma)     # (a NaN rejects)
            c, ev, init = rq.event_rule(c, True, accepted, rq.initial_state_is_finite(model, meas[s, j]), K)
            out["event"][s, j] = ev
            if accepted:
                out["acc"][s, j] = True
                t.add_measurement(dt, meas[s, j])
            elif init:
                t = tw.Target(model, Q, R, P0, meas[s, j], DT)
            else:
                t.update(dt)
        out["x"][j], out["P"][j], out["run"][j] = t.x, t.P, c
    return out


@functools.lru_cache(maxsize=None)
def twin(name, gamma, K):
    """the twin over reacquire_ref.stream(name) stepped at SCHEDULE, computed once and shared, read-only"""
    import oracle
    from conftest import model_path
    mdl = oracle.load_model_yaml(model_path(name))
    p0, meas, mask, _, _ = rq.stream(name)
    out = twin_schedule(mdl["model"], mdl["Q"], mdl["R"], mdl["P"], p0, meas, mask, SCHEDULE, gamma, K)
    for v in out.values():
        v.setflags(write=False)
    return out
