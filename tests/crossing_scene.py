"""The scene of the crossing-covariance tests (CPU and GPU): n targets outside a sphere, four fifths of them heading inward so that
they cross it, a fixed fifth aimed to miss, filtered for TICKS ticks under a has-mask that leaves some 64-target tiles fully
measured and splits others.  Also the oracle side of the comparison: Sigma as the position block a predict-only step by tau
leaves, and sigma_r / sigma_t from it in NumPy longdouble."""
import ctypes as C

import numpy as np

ORIGIN = np.array([0.5, -0.25, 0.3])
RADIUS = 1.5
TICKS = 12
DT = 0.004
NOISE = 1e-4          # metres: the estimates stay near the truth, so who crosses is the scene's decision, not the noise's
CROSSING_MODELS = ("uniform_acceleration", "angular_rates")   # the query never crosses for the constant-velocity models


def aimed_to_miss(n):
    """the fixed fifth: targets 2, 7, 12, ..."""
    return np.arange(n) % 5 == 2


def has_mask(n):
    """[TICKS, n] uint8: tiles 0, 2, 4, ... (64 targets each) are measured on every tick; in the odd tiles the targets 3 mod 7 miss
    the ticks 1 mod 4, which splits those tiles (for n <= 64 there is only tile 0: every target measured on every tick)"""
    has = np.ones((TICKS, n), dtype=np.uint8)
    i = np.arange(n)
    split = ((i // 64) % 2 == 1) & (i % 7 == 3)
    for s in range(TICKS):
        if s % 4 == 1:
            has[s, split] = 0
    return has


def build(n, seed=2026):
    """dict(p0 [n,7], v0 [n,6], a0 [n,6], meas [TICKS,n,7], has [TICKS,n], miss [n]).  A crosser starts 6..9 m from the origin of
    the sphere on a seeded direction and closes at 8..12 m/s along the line through a point within 0.5 m of the sphere's centre,
    decelerating by 1..3 m/s^2: it reaches the sphere (1.5 m) after 0.4..0.9 s, still faster than 7 m/s, well inside 20 degrees
    of the normal.  A target aimed to miss moves and accelerates outward along its own radius: its distance only grows."""
    rng = np.random.default_rng(seed + n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    start = ORIGIN + u * rng.uniform(6.0, 9.0, (n, 1))
    aim = ORIGIN + rng.uniform(-0.5, 0.5, (n, 3)) / np.sqrt(3.0)
    w = aim - start
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    speed = rng.uniform(8.0, 12.0, (n, 1))
    decel = rng.uniform(1.0, 3.0, (n, 1))
    vel, acc = w * speed, -w * decel
    miss = aimed_to_miss(n)
    vel[miss] = u[miss] * speed[miss]
    acc[miss] = u[miss] * decel[miss]
    p0 = np.zeros((n, 7)); p0[:, :3] = start; p0[:, 6] = 1.0
    v0 = np.zeros((n, 6)); v0[:, :3] = vel
    a0 = np.zeros((n, 6)); a0[:, :3] = acc
    meas = np.zeros((TICKS, n, 7))
    for s in range(TICKS):
        t = DT * (s + 1)
        meas[s, :, :3] = start + vel * t + 0.5 * acc * t * t + rng.normal(0.0, NOISE, (n, 3))
        meas[s, :, 6] = 1.0
    return dict(p0=p0, v0=v0, a0=a0, meas=meas, has=has_mask(n), miss=miss)


def oracle_batch(oracle, model, scene, dtype="f64", Q=None, R=None, P0=None):
    """the oracle's targets of the scene, filtered for TICKS ticks under the mask"""
    orc = oracle.OracleBatch(model["model"], model["Q"] if Q is None else Q, model["R"] if R is None else R,
                             model["P"] if P0 is None else P0, scene["p0"], DT, 0.0, scene["v0"], scene["a0"], dtype=dtype)
    for s in range(TICKS):
        orc.step(DT, scene["meas"][s], scene["has"][s])
    return orc


def _one(orc, i):
    """a copy of target i as a batch of one (the oracle's targets are plain structs: it copies them by value itself)"""
    one = object.__new__(type(orc))
    one.__dict__.update(orc.__dict__)
    one.N = 1
    one.buf = (C.c_char * orc.size)()
    one.base = C.addressof(one.buf)
    C.memmove(one.base, orc.base + i * orc.size, orc.size)
    return one


def oracle_rows(orc, delta, t1=None):
    """For every target i with delta[i] >= 0: a copy of the oracle's target stepped predict-only by tau_i = delta[i] + (t1 - t_i)
    (t1 None: its own time), and from it Sigma = P^-[0:3, 0:3] [n,3,3], scale = max|P^-| [n], p_c, v_c = pose_at / twist_at of
    the unstepped target at t_i + tau_i [n,3].  Rows of the others are NaN."""
    n = orc.N
    times = orc.times()
    Sigma = np.full((n, 3, 3), np.nan); scale = np.full(n, np.nan); pc = np.full((n, 3), np.nan); vc = np.full((n, 3), np.nan)
    tau = np.full(n, np.nan)
    for i in range(n):
        if not delta[i] >= 0:
            continue
        dq = 0.0 if t1 is None else t1 - times[i]
        tau[i] = delta[i] + dq
        one = _one(orc, i)
        pc[i] = one.pose_at(times[i] + tau[i])[0, :3]
        vc[i] = one.twist_at(times[i] + tau[i])[0, :3]
        one.step(tau[i], None)
        P = one.state()[1][0]
        Sigma[i] = P[:3, :3]
        scale[i] = np.abs(P).max()
    return dict(Sigma=Sigma, scale=scale, pc=pc, vc=vc, tau=tau)


def sigma_reference(Sigma, pc, vc, origin=ORIGIN):
    """sigma_r, sigma_t, |n . v_c|, |p_c - o|, n^T Sigma n per row, in NumPy longdouble"""
    L = np.longdouble
    d = pc.astype(L) - origin.astype(L)
    dist = np.sqrt((d * d).sum(axis=1))
    nrm = d / dist[:, None]
    form = np.einsum("ni,nij,nj->n", nrm, Sigma.astype(L), nrm)
    nv = np.abs((nrm * vc.astype(L)).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        sr = np.sqrt(form)
        st = sr / nv
    return sr, st, nv, dist, form
