"""Reference, streams and outliers for the NIS validation gate (tests/test_gate_reference.py, tests/test_gpu_gate.py).

Built on tests/innov_stream_ref.py: one oracle/np_twin.py Target per target; before each measurement nu, S^-1 and NIS are formed
as twin_innovations forms them, then add_measurement if nis <= gamma and update(dt) otherwise -- update(dt) leaves the twin's
meas_rpy (the unwrap memory) alone.

The streams are those of the innovation tests -- synth_stream(name, 203, 20, seed=31), innov_stream_ref.masks(20, 203, 31),
dt 0.004 -- with outliers added:
  * on a Bernoulli(1/12) subset of the measured (tick, target) pairs from tick 2 on, drawn with default_rng(5): +0.5 m on one of
    x / y / z;
  * angular models: on two targets a yaw measurement rotated by +2.9 rad on tick 6 and by +3.6 rad on tick 7, clean after (the
    yaw variance of the shipped R puts 2.5 rad at NIS 551 and 5.0 rad -- 1.28 rad once wrapped -- at 148, below gamma = 300).  If the
    unwrap memory advanced on the first rejection, the second spike would unwrap to another branch and the clean measurement
    behind it would be off by 2 pi."""
import functools

import numpy as np

import innov_stream_ref as ref
from oracle import np_twin as tw

N, TICKS, SEED, DT = 203, 20, 31, 0.004
GAMMA_FAR = 300.0                      # far from every NIS of the stream (tests/test_gate_reference.py asserts the margin)
CHI2_99 = {3: 11.345, 6: 16.812}       # the 0.99 quantile of chi-square with m degrees of freedom
SPIKE_TICKS, SPIKE_ANGLES = (6, 7), (2.9, 3.6)


def m_of(name):
    return 6 if name.startswith("angular") else 3


def _yaw_rotated(q, angle):
    c, s = np.cos(angle), np.sin(angle)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return tw.quat_normalize(tw.rot_to_quat(Rz @ tw.quat_to_rot(tw.quat_normalize(q))))


@functools.lru_cache(maxsize=None)
def stream(name):
    """p0 [N,7], meas [TICKS,N,7] with the outliers, mask [TICKS,N], outlier [TICKS,N] bool (the +0.5 m pairs), spikes: a list of
    (tick, target) yaw-spike pairs (angular models).  Read-only, shared."""
    p0, clean, mask, _ = ref.stream_and_reference(name, N, TICKS, SEED)
    meas = clean.copy()
    has = mask.astype(bool)
    rng = np.random.default_rng(5)
    outlier = has & (rng.random((TICKS, N)) < 1.0 / 12.0)
    outlier[:2] = False
    axis = rng.integers(0, 3, (TICKS, N))
    for s, j in zip(*np.nonzero(outlier)):
        meas[s, j, axis[s, j]] += 0.5
    spikes = []
    if m_of(name) == 6:
        # the first two targets that are measured, without a position outlier, on the spike ticks and the two ticks behind them
        span = range(SPIKE_TICKS[0], SPIKE_TICKS[-1] + 3)
        ok = [j for j in range(N) if all(has[s, j] and not outlier[s, j] for s in span)][:2]
        assert len(ok) == 2
        for j in ok:
            for s, a in zip(SPIKE_TICKS, SPIKE_ANGLES):
                meas[s, j, 3:7] = _yaw_rotated(meas[s, j, 3:7], a)
                spikes.append((s, j))
    for v in (meas, outlier):
        v.setflags(write=False)
    return p0, meas, mask, outlier, tuple(spikes)


def twin_gated(model, Q, R, P0, p0, meas, mask, dt, gamma):
    """innov_stream_ref.twin_innovations with the gate: the same dict (nu, nis, xm, w, Sinv, pmax of every measured pair, accepted
    or not; x, P at the end) plus acc [ticks, N] bool."""
    ticks, n_t = meas.shape[0], meas.shape[1]
    n, m = tw.DIMS[model]
    out = dict(nu=np.zeros((ticks, n_t, m)), nis=np.full((ticks, n_t), -1.0), xm=np.zeros((ticks, n_t, m)), w=np.zeros((ticks, n_t, m)),
               Sinv=np.zeros((ticks, n_t, m, m)), pmax=np.zeros((ticks, n_t)), x=np.zeros((n_t, n)), P=np.zeros((n_t, n, n)),
               acc=np.zeros((ticks, n_t), bool))
    for j in range(n_t):
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
            nis = nu @ w
            out["nu"][s, j], out["nis"][s, j], out["xm"][s, j], out["w"][s, j] = nu, nis, xm[:m], w
            out["Sinv"][s, j], out["pmax"][s, j] = Sinv, np.abs(Pm).max()
            if nis <= gamma:     # (a NaN rejects)
                out["acc"][s, j] = True
                t.add_measurement(dt, meas[s, j])
            else:
                t.update(dt)
        out["x"][j], out["P"][j] = t.x, t.P
    return out


@functools.lru_cache(maxsize=None)
def reference(name, gamma):
    """the gated twin over stream(name) at `gamma`, computed once and shared, read-only"""
    import oracle
    from conftest import model_path
    mdl = oracle.load_model_yaml(model_path(name))
    p0, meas, mask, _, _ = stream(name)
    out = twin_gated(mdl["model"], mdl["Q"], mdl["R"], mdl["P"], p0, meas, mask, DT, gamma)
    for v in out.values():
        v.setflags(write=False)
    return out


def margin(want, mask, dtype, gamma):
    """|NIS - gamma| over the innov_stream_ref bound, [ticks, N]; inf where the target has no measurement"""
    _, nb = ref.bounds(want, dtype)
    has = mask.astype(bool)
    r = np.full(mask.shape, np.inf)
    r[has] = np.abs(want["nis"][has] - gamma) / nb[has]
    return r
