"""NumPy twin of the association of unlabelled detections (csrc/associate_plan.hpp, csrc/associate.hip).

table(): the per-target row (zhat, S, W) from a state x, a covariance P and the class matrices -- in float64 / float32 in the kernel's
statement order (a fused multiply-add of the kernel is a multiply and an add here: NumPy has none), or in longdouble.  d2(): the pair
costs.  match(): the rounds of mutual best, exactly the device's rule.  greedy(): sorted greedy global-nearest-neighbour, what the
rounds reach at their fixed point.  chain(): the scene that matches exactly one pair per round."""
import numpy as np

MODEL_NK = {"uniform_velocity": (6, 3), "uniform_acceleration": (9, 3), "angular_rates": (18, 6), "angular_velocities": (12, 6)}
MAX_ROUNDS = 16
MAX_DETECTIONS = 65536


def _wide(T):
    return np.longdouble if T is np.longdouble else np.float64


def table(x, P, Q, R, dt, name, T=np.float64):
    """x [n, N], P [n, N, N], Q [N, N] or [n, N, N], R [m, m] or [n, m, m] (the slot's class) -> zhat [n, 3], S [n, 3, 3], W [n, 3, 3],
    valid [n].  zhat and Sigma in T; S = Sigma + R[0:3, 0:3] and W = S^-1 (cofactors) in double (longdouble for T = longdouble).
    An invalid S (not finite, a non-positive diagonal entry or determinant) gives NaN rows."""
    N, K = MODEL_NK[name]
    NB = N // K
    n = x.shape[0]
    W_ = _wide(T)
    x = np.asarray(x).astype(T)
    P = np.asarray(P).astype(T)
    Q = np.broadcast_to(np.asarray(Q), (n, N, N)).astype(T)
    R = np.asarray(R)
    R = np.broadcast_to(R, (n,) + R.shape[-2:]).astype(T)
    d = T(dt)
    hdt = T(0.5) * d * d
    # derive_outputs: x + v d (+ 0.5 a d d), left to right
    zhat = x[:, 0:3] + x[:, K:K + 3] * d
    if NB == 3:
        zhat = zhat + T(0.5) * x[:, 2 * K:2 * K + 3] * d * d
    S = np.zeros((n, 3, 3), dtype=W_)
    for r in range(3):
        for c in range(r, 3):
            B = np.stack([np.stack([P[:, r + i * K, c + j * K] for j in range(NB)], axis=1) for i in range(NB)], axis=1)   # [n, NB, NB]
            Qb = np.stack([np.stack([Q[:, r + i * K, c + j * K] for j in range(NB)], axis=1) for i in range(NB)], axis=1)
            B = B.copy()
            for b in range(NB - 1):        # crossing_predict_block: rows ...
                for cc in range(NB):
                    v = d * B[:, b + 1, cc] + B[:, b, cc]
                    if NB == 3 and b == 0:
                        v = hdt * B[:, b + 2, cc] + v
                    B[:, b, cc] = v
            v = B[:, 0, 0]                 # ... then columns, entry [0][0] only, + Q
            if NB > 1:
                v = d * B[:, 0, 1] + v
                if NB == 3:
                    v = hdt * B[:, 0, 2] + v
            v = v + Qb[:, 0, 0]
            S[:, r, c] = v.astype(W_) + R[:, r, c].astype(W_)
            S[:, c, r] = S[:, r, c]
    W, valid = invert(S)
    zhat = zhat.astype(W_)
    zhat[~valid] = np.nan
    return zhat, S, W, valid


def invert(S):
    """assoc_invert_s over [n, 3, 3]: cofactors in S's own type, the validity rule; invalid rows NaN"""
    s0, s1, s2, s3, s4, s5 = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    with np.errstate(all="ignore"):
        c00 = s3 * s5 - s4 * s4
        c01 = s2 * s4 - s1 * s5
        c02 = s1 * s4 - s2 * s3
        c11 = s0 * s5 - s2 * s2
        c12 = s1 * s2 - s0 * s4
        c22 = s0 * s3 - s1 * s1
        det = (s0 * c00 + s1 * c01) + s2 * c02
        valid = np.isfinite(S).all(axis=(1, 2)) & (s0 > 0) & (s3 > 0) & (s5 > 0) & (det > 0) & np.isfinite(det)
        W = np.empty_like(S)
        W[:, 0, 0] = c00 / det; W[:, 0, 1] = W[:, 1, 0] = c01 / det; W[:, 0, 2] = W[:, 2, 0] = c02 / det
        W[:, 1, 1] = c11 / det; W[:, 1, 2] = W[:, 2, 1] = c12 / det; W[:, 2, 2] = c22 / det
    W[~valid] = np.nan
    return W, valid


def d2(zhat, W, det):
    """assoc_d2 for every pair: [n, M], in the type of zhat / W (double or longdouble); det [M, >= 3]"""
    T = zhat.dtype.type
    z = np.asarray(det)[:, 0:3].astype(T)
    with np.errstate(all="ignore"):
        nx = z[None, :, 0] - zhat[:, None, 0]
        ny = z[None, :, 1] - zhat[:, None, 1]
        nz = z[None, :, 2] - zhat[:, None, 2]
        w = lambda r, c: W[:, r, c][:, None]
        t0 = (w(0, 0) * nx + w(0, 1) * ny) + w(0, 2) * nz
        t1 = (w(0, 1) * nx + w(1, 1) * ny) + w(1, 2) * nz
        t2 = (w(0, 2) * nx + w(1, 2) * ny) + w(2, 2) * nz
        return (nx * t0 + ny * t1) + nz * t2


def _pick(D, free, axis):
    """per row (axis = 1) or column (axis = 0): the index of the smallest free entry, the lowest index among equals; -1: none"""
    key = np.where(free, D, np.inf)
    idx = np.argmin(key, axis=axis)
    has = free.any(axis=axis)
    taken = np.take_along_axis(free, np.expand_dims(idx, axis), axis).squeeze(axis)
    for e in np.nonzero(has & ~taken)[0]:      # the minimum is +inf and a non-free entry came first: the first free +inf
        line = free[e] if axis == 1 else free[:, e]
        idx[e] = int(np.nonzero(line)[0][0])
    return np.where(has, idx, -1)


def match(D, gate, rounds):
    """The device's rounds on the cost matrix D [rows, M] (rows in (batch, slot) order; NaN: never a candidate).
    Returns det_of_row [rows], row_of_det [M], info = [matched, rounds_run, settled, 0]."""
    D = np.asarray(D, dtype=np.float64)
    n, M = D.shape
    det_of_row = np.full(n, -1, dtype=np.int64)
    row_of_det = np.full(M, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        cand = D <= gate
    matched, run, settled = 0, 0, int(n == 0 or M == 0)
    for _ in range(rounds):
        if settled:
            break
        free = cand & (det_of_row < 0)[:, None] & (row_of_det < 0)[None, :]
        pick_r = _pick(D, free, 1)
        pick_d = _pick(D, free, 0)
        open_ = 0
        for j in range(M):
            if row_of_det[j] >= 0 or pick_d[j] < 0:
                continue
            i = pick_d[j]
            if pick_r[i] == j:
                row_of_det[j] = i; det_of_row[i] = j
                matched += 1
            else:
                open_ += 1
        run += 1
        settled = int(open_ == 0)
    return det_of_row, row_of_det, [matched, run, settled, 0]


def greedy(D, gate):
    """sorted greedy global-nearest-neighbour: pairs by (d2, row, detection), each taken if its row and column are free"""
    D = np.asarray(D, dtype=np.float64)
    n, M = D.shape
    det_of_row = np.full(n, -1, dtype=np.int64)
    row_of_det = np.full(M, -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ii, jj = np.nonzero(D <= gate)
    order = np.lexsort((jj, ii, D[ii, jj]))
    for k in order:
        i, j = ii[k], jj[k]
        if det_of_row[i] < 0 and row_of_det[j] < 0:
            det_of_row[i] = j; row_of_det[j] = i
    return det_of_row, row_of_det


def chain(L):
    """points on the x axis alternating target, detection, target, ... with strictly decreasing integer gaps: with equal S and a
    wide gate exactly one pair is matched per round, from the far end; settled only at round L.  Returns (targets [L], dets [L])."""
    gaps = np.arange(2 * L - 1, 0, -1, dtype=np.float64) + 1.0     # 2L, 2L - 1, ..., 2
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    return pos[0::2].copy(), pos[1::2].copy()
