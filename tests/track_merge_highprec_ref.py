"""An independent extended-precision reference of the duplicate-track search's numbers, written from the model
definitions and from linear algebra, not from the kernels: nothing here is shared with associate_ref.table / invert / d2 or with
track_merge_ref.pair_terms, there is no cofactor and no block-by-block predict.

rows(): zhat = (A(dt) x)[0:3] and Sigma = (A(dt) P A(dt)^T + Q)[0:3, 0:3] from the dense N x N products, A(dt) written out per
model.  pairs(): C = Sigma_lo + Sigma_hi, its Cholesky factor, d2 = nu^T C^-1 nu through two triangular solves; a C whose
factorisation fails gives NaN: no candidate.  decide(): the classes, the pair box and the gate on those numbers -- the cost matrix
the matching runs on.  greedy(): sorted greedy over pairs by (d2, lo, hi), the fixed point of the rounds.  Everything in
numpy.longdouble (64-bit significand: u = 2^-64)."""
import numpy as np

L = np.longdouble
MODEL_NK = {"uniform_velocity": (6, 3), "uniform_acceleration": (9, 3), "angular_rates": (18, 6), "angular_velocities": (12, 6)}
NONE, ELIGIBLE, WIDE = 0, 1, 2


def transition(dt, name):
    """A(dt) [N, N] in longdouble.  uniform_velocity: x = (p, v), p' = p + v dt.  uniform_acceleration: x = (p, v, a), p' = p + v dt
    + a dt^2 / 2, v' = v + a dt.  angular_rates: the same chain over the six pose words (position and roll-pitch-yaw).
    angular_velocities: x = (pose6, twist6), p' = p + v dt; its attitude rows are a state-dependent Jacobian that only reaches rows
    and columns 3..5 of A P A^T, never the position block asked for here: they are left as the identity."""
    N, K = MODEL_NK[name]
    d = L(dt)
    A = np.eye(N, dtype=L)
    i = np.arange(N)
    if name == "uniform_velocity":
        A[i[:3], i[:3] + 3] = d
    elif name in ("uniform_acceleration", "angular_rates"):
        A[i[:2 * K], i[:2 * K] + K] = d
        A[i[:K], i[:K] + 2 * K] = d * d / L(2)
    else:
        A[i[:3], i[:3] + K] = d
    return A


def rows(x, P, Q, dt, name, R=None):
    """x [n, N], P [n, N, N], Q [N, N] or [n, N, N] (R [m, m] or [n, m, m], optional) -> zhat [n, 3], Sigma [n, 3, 3], valid [n].
    valid: Sigma is finite and, where R is given, S = Sigma + R[0:3, 0:3] has a Cholesky factor (the association's row exists)."""
    N, K = MODEL_NK[name]
    x, P = np.asarray(x).astype(L), np.asarray(P).astype(L)
    n = x.shape[0]
    Q = np.broadcast_to(np.asarray(Q), (n, N, N)).astype(L)
    A = transition(dt, name)
    with np.errstate(all="ignore"):
        zhat = (x @ A.T)[:, 0:3]
        full = np.matmul(np.matmul(A[None], P), A.T[None]) + Q
    Sigma = full[:, 0:3, 0:3]
    Sigma = (Sigma + np.swapaxes(Sigma, 1, 2)) / L(2)
    valid = np.isfinite(Sigma.astype(np.float64)).all(axis=(1, 2)) & np.isfinite(zhat.astype(np.float64)).all(axis=1)
    if R is not None:
        R = np.asarray(R)
        R = np.broadcast_to(R, (n,) + R.shape[-2:]).astype(L)
        _, ok = cholesky(Sigma + R[:, 0:3, 0:3])
        valid = valid & ok
    return zhat, Sigma, valid


def cholesky(C):
    """C [..., 3, 3] symmetric -> the lower factor G [..., 3, 3] with C = G G^T, and ok [...]: every pivot finite and positive"""
    C = np.asarray(C).astype(L)
    G = np.zeros_like(C)
    ok = np.ones(C.shape[:-2], dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(3):
            piv = C[..., j, j] - sum((G[..., j, k] * G[..., j, k] for k in range(j)), L(0))
            good = np.isfinite(piv.astype(np.float64)) & (piv > 0)
            ok &= good
            G[..., j, j] = np.sqrt(np.where(good, piv, L(1)))
            for i in range(j + 1, 3):
                G[..., i, j] = (C[..., i, j] - sum((G[..., i, k] * G[..., j, k] for k in range(j)), L(0))) / G[..., j, j]
    return G, ok


def solve_quadratic_form(G, nu):
    """nu^T (G G^T)^-1 nu: G y = nu forwards, G^T w = y backwards, then nu . w"""
    y = [None] * 3
    for i in range(3):
        y[i] = (nu[..., i] - sum((G[..., i, k] * y[k] for k in range(i)), L(0))) / G[..., i, i]
    w = [None] * 3
    for i in (2, 1, 0):
        w[i] = (y[i] - sum((G[..., k, i] * w[k] for k in range(i + 1, 3)), L(0))) / G[..., i, i]
    return nu[..., 0] * w[0] + nu[..., 1] * w[1] + nu[..., 2] * w[2]


def pairs(zhat, Sigma):
    """for every pair, both ways round: C [n, n, 3, 3], nu [n, n, 3] (z_j - z_i), d2 [n, n] (NaN: C has no Cholesky factor; NaN
    on the diagonal)"""
    zhat, Sigma = np.asarray(zhat).astype(L), np.asarray(Sigma).astype(L)
    n = zhat.shape[0]
    with np.errstate(all="ignore"):
        C = Sigma[:, None] + Sigma[None, :]
        nu = zhat[None, :, :] - zhat[:, None, :]
        G, ok = cholesky(C)
        d2 = solve_quadratic_form(G, nu)
    d2 = np.where(ok, d2, L("nan"))
    if n:
        d2[np.arange(n), np.arange(n)] = L("nan")
    return C, nu, d2


def reach2(gate, s):
    """the box of the project: gate s (1 + 2^-10), here without rounding to double"""
    return L(gate) * np.asarray(s).astype(L) * (L(1) + L(2) ** -10)


def narrow_limit2(cell):
    lim = L(cell) * (L(1) - L(2) ** -20)
    return lim * lim


def classes(Sigma, valid, hits, min_hits, gate, cell):
    """[n]: NONE (invalid, or hits < min_hits), ELIGIBLE (the row's own box, reach2(gate, 2 Sigma_aa), within a cell on every axis), WIDE"""
    diag = np.stack([Sigma[:, a, a] for a in range(3)], axis=1)
    with np.errstate(invalid="ignore"):
        narrow = (reach2(gate, 2 * diag) <= narrow_limit2(cell)).all(axis=1)
    ok = np.asarray(valid, dtype=bool) & (np.asarray(hits).astype(np.int64) >= int(min_hits))
    return np.where(ok, np.where(narrow, ELIGIBLE, WIDE), NONE)


def box(C, nu, gate):
    """[n, n] bool: nu_a^2 <= reach2(gate, C_aa) on every axis"""
    ok = np.ones(nu.shape[:2], dtype=bool)
    with np.errstate(invalid="ignore"):
        for a in range(3):
            ok &= nu[..., a] * nu[..., a] <= reach2(gate, C[..., a, a])
    return ok


def decide(zhat, Sigma, valid, hits, min_hits, gate, cell):
    """the cost matrix [n, n] in double (NaN: no candidate) and the classes"""
    C, nu, d2 = pairs(zhat, Sigma)
    cls = classes(Sigma, valid, hits, min_hits, gate, cell)
    e = cls == ELIGIBLE
    with np.errstate(invalid="ignore"):
        cand = e[:, None] & e[None, :] & (d2 <= L(gate)) & box(C, nu, gate)
    return np.where(cand, d2, L("nan")).astype(np.float64), cls


def greedy(D):
    """sorted greedy over the pairs lo < hi of a cost matrix by (d2, lo, hi): partner [n] (-1: none)"""
    n = len(D)
    items = sorted((float(D[lo][hi]), lo, hi) for lo in range(n) for hi in range(lo + 1, n) if D[lo][hi] == D[lo][hi])
    partner = [-1] * n
    for _, lo, hi in items:
        if partner[lo] < 0 and partner[hi] < 0:
            partner[lo], partner[hi] = hi, lo
    return np.array(partner, dtype=np.int64)


def cond(C):
    """the 2-norm condition number of every symmetric 3 x 3 (double is enough for a figure that is only reported and binned)"""
    w = np.linalg.eigvalsh(np.asarray(C, dtype=np.float64))
    with np.errstate(all="ignore"):
        return np.where(w[..., 0] > 0, w[..., 2] / w[..., 0], np.inf)


def deviation(d2, ref, window):
    """the largest |d2 - ref| / max(ref, 1) over the pairs whose reference is finite and <= window; 0.0 if there is none"""
    ref = np.asarray(ref).astype(L)
    with np.errstate(invalid="ignore"):
        m = np.isfinite(ref.astype(np.float64)) & (ref <= L(window))
    if not m.any():
        return 0.0
    got = np.asarray(d2).astype(L)[m]
    assert np.isfinite(got.astype(np.float64)).all()           # a pair the reference factorises has a cost
    return float((np.abs(got - ref[m]) / np.maximum(ref[m], L(1))).max())


def allowance(dev):
    """8 x the same-precision twin's deviation from this reference, never below 2^-50: the yardstick of a device d2"""
    return max(8.0 * dev, 2.0 ** -50)


def separation(zhat, Sigma, valid, gate, cell):
    """the smallest relative margins of a scene, over the valid rows: (gap, box, cls).  gap: between any two d2 <= 4 gate and
    between any of them and the gate, relative to max(d2, 1).  box: |nu_a^2 / reach2_a - 1| over the pairs with d2 <= 4 gate (no
    other pair can become a candidate whatever its box says).  cls: |reach2_a / limit2 - 1| over the rows."""
    v = np.asarray(valid, dtype=bool)
    C, nu, d2 = pairs(zhat, Sigma)
    n = len(v)
    up = np.triu(np.ones((n, n), dtype=bool), 1) & v[:, None] & v[None, :]
    with np.errstate(invalid="ignore"):
        near = up & (d2 <= L(4 * gate))
    vals = np.sort(d2[near].astype(np.float64))
    gap = np.inf
    if len(vals) > 1:
        gap = float((np.diff(vals) / np.maximum(vals[1:], 1.0)).min())
    if len(vals):
        gap = min(gap, float((np.abs(vals - gate) / max(gate, 1.0)).min()))
    bx = np.inf
    for a in range(3):
        r = (nu[..., a] * nu[..., a] / reach2(gate, C[..., a, a]))[near]
        if r.size:
            bx = min(bx, float(np.abs(r - 1).min()))
    diag = np.stack([Sigma[:, a, a] for a in range(3)], axis=1)[v]
    cl = float(np.abs(reach2(gate, 2 * diag) / narrow_limit2(cell) - 1).min()) if v.any() else np.inf
    return gap, bx, cl
