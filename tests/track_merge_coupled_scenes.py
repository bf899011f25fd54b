"""Coupled scenes for the duplicate-track search: what no fresh diagonal world gives it.  No GPU, no library.

Every target has a dense SPD covariance: its position block is 0.0025 U diag(r^2, 1, r^-2) U^T in a random frame U (5 cm across,
axis ratio r^2, cond = r^4), every other block is populated through P = [I X]^T Sigma_pp [I X] + blkdiag(0, V) with X dense
(position-position, position-velocity, position-acceleration, position-attitude words, all across axes) and V dense SPD.  Q is
dense SPD.  The velocity and, for the models that have one, the acceleration state are non-zero.  Rows come in families of four:
row 4f + 1 is a TWIN of row 4f (its covariance the predecessor's under a congruence 1e-3 from the identity, its position the
predecessor's predicted position plus an offset whose d2 is planted), every second family has a third track next to the twin, a few
rows are wide (their covariance scaled by a power of two) and a few have too few hits.  Positions, velocities and accelerations
lie on binary grids so that at dt = 2^-6 the predicted position is exact in the batch's precision."""
from types import SimpleNamespace

import numpy as np

import track_merge_highprec_ref as hp

GATE = 9.0
MIN_HITS = 2
RATIOS = {"f64": (1.0, 12.0, 3.0, 30.0, 12.0, 30.0), "f32": (1.0, 1.6, 2.5)}      # cond(Sigma_pp) = r^4: up to 8.1e5, and up to 39
CELL = {"f64": 8.0, "f32": 0.75}                                       # the narrow rows' reach: below 6.4 m, below 0.6 m
WIDE_SCALE = {"f64": 2.0 ** 12, "f32": 2.0 ** 6}


def np_t(dtype):
    return np.float32 if dtype == "f32" else np.float64


def _grid(a, step):
    return np.round(np.asarray(a) / step) * step


def _dense_spd(rng, m, scale):
    M = rng.normal(size=(m, m))
    return scale * (np.eye(m) + 0.5 * (M @ M.T) / m)


def coupled_q(name, scale=1e-7):
    """dense SPD process noise: every word between two axes and two derivatives populated"""
    N, _ = hp.MODEL_NK[name]
    return _dense_spd(np.random.default_rng(4242 + N), N, scale)


def coupled_p(rng, name, r, scale=0.0025, cross=0.2, rest=1e-6):
    N, _ = hp.MODEL_NK[name]
    U, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Spp = scale * (U @ np.diag([r * r, 1.0, 1.0 / (r * r)]) @ U.T)
    J = np.concatenate([np.eye(3), cross * rng.normal(size=(3, N - 3))], axis=1)        # [3, N]: [I X]
    P = J.T @ Spp @ J
    P[3:, 3:] += _dense_spd(rng, N - 3, rest)
    # (the rows in the model's order: the position words are 0..2 in every model)
    return 0.5 * (P + P.T)


def state(name, pos, vel, acc):
    """x [n, N] of fresh targets: position, linear velocity and (NB = 3) linear acceleration on their chains, the rest zero"""
    N, K = hp.MODEL_NK[name]
    n = len(pos)
    x = np.zeros((n, N))
    x[:, 0:3] = pos
    x[:, K:K + 3] = vel
    if N // K == 3:
        x[:, 2 * K:2 * K + 3] = acc
    return x


def counters(n):
    """row 4f + 3 of every third family and row 5 (a twin) below MIN_HITS; the others 2 .. 4 hits; some misses"""
    i = np.arange(n)
    low = ((i % 4 == 3) & ((i // 4) % 3 == 0)) | (i == 5)
    hits = np.where(low, 1, 2 + i % 3).astype(np.uint8)
    miss = ((i // 3) % 3).astype(np.uint8)
    return hits, miss


def scene(name, dtype, n, seed, dt, spacing=1.0, origin=(0.0, 0.0, 0.0), third=True):
    """pos, vel, acc [n, 3], P0 [n, N, N], Q [N, N] -- all rounded to the batch's precision, as a device batch holds them -- and
    ratio [n], wide [n].  The twins' offsets are planted against the reference's Sigma at `dt`: d2 in an arithmetic progression
    over (0.05, 0.9 gate), every tenth over (1.1, 3.5) gate."""
    T = np_t(dtype)
    rng = np.random.default_rng(seed)
    N, K = hp.MODEL_NK[name]
    i = np.arange(n)
    step = 2.0 ** -10 if dtype == "f32" else 2.0 ** -30
    pos = np.stack([i % 8, (i // 8) % 8, i // 64], axis=1) * spacing + np.asarray(origin) + rng.uniform(-0.2, 0.2, (n, 3)) * spacing
    pos = _grid(pos, 2.0 ** -10)
    vel = _grid(rng.uniform(-2, 2, (n, 3)), 2.0 ** -4)
    acc = _grid(rng.uniform(-3, 3, (n, 3)), 2.0 ** -4)
    acc[acc == 0.0] = 2.0 ** -4
    Q = coupled_q(name).astype(T).astype(np.float64)
    ratios = RATIOS[dtype]
    ratio = np.array([ratios[(k // 4) % len(ratios)] for k in range(n)])
    P0 = np.zeros((n, N, N))
    wide = (i % 4 == 2) & ((i // 4) % 4 == 1) | (i == 13)
    for k in range(n):
        if k % 4 == 1 or (third and k % 8 == 2):            # the predecessor's covariance, slightly perturbed
            G = np.eye(N) + 1e-3 * rng.normal(size=(N, N))
            assert not wide[k - 1]
            P0[k] = G @ P0[k - 1] @ G.T
        else:
            P0[k] = coupled_p(rng, name, ratio[k])
        P0[k] = 0.5 * (P0[k] + P0[k].T)
        if wide[k]:
            P0[k] *= WIDE_SCALE[dtype]
    P0 = P0.astype(T).astype(np.float64)
    # the twins: placed where the PREDICTED positions differ by the planted offset (same velocity and acceleration)
    follow = [k for k in range(1, n) if k % 4 == 1 or (third and k % 8 == 2)]
    vals = 0.05 + (np.arange(len(follow)) + 0.5) * (0.85 * GATE / max(len(follow), 1))
    vals[4::10] = GATE * (1.1 + 2.4 * rng.uniform(size=len(vals[4::10])))
    vals = rng.permutation(vals)
    x = state(name, pos, vel, acc)
    _, Sigma, _ = hp.rows(x, P0, Q, dt, name)
    Sigma = Sigma.astype(np.float64)
    for v, k in zip(vals, follow):
        vel[k], acc[k] = vel[k - 1], acc[k - 1]
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        Lc = np.linalg.cholesky(Sigma[k - 1] + Sigma[k])
        pos[k] = _grid(pos[k - 1] + Lc @ u * np.sqrt(v), step)
    for a in (pos, vel, acc):
        assert np.array_equal(a.astype(T).astype(np.float64), a)                # representable in the batch's precision
    return SimpleNamespace(name=name, dtype=dtype, n=n, pos=pos, vel=vel, acc=acc, P0=P0, Q=Q, ratio=ratio, wide=wide,
                           x=state(name, pos, vel, acc))


def fill_world(w, s):
    """a test_gpu_associate.World takes the scene's targets"""
    w.p0[:, :3] = s.pos
    w.v0[:] = 0.0; w.v0[:, :3] = s.vel
    w.a0[:] = 0.0; w.a0[:, :3] = s.acc
    w.P0, w.Q = s.P0, s.Q
    return w


def correlation(C):
    """[...]: the largest |C_ab| / sqrt(C_aa C_bb) over the three axis pairs"""
    C = np.asarray(C, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.max([np.abs(C[..., a, b]) / np.sqrt(C[..., a, a] * C[..., b, b]) for a, b in ((0, 1), (0, 2), (1, 2))], axis=0)
