"""NumPy twin of the grid form of the association (csrc/associate_grid_plan.hpp, csrc/associate_grid.hip).

The table, d2 and the rounds are associate_ref's.  This module adds what the grid form adds: the box rule (reach2, a mask over the
cost matrix), the narrow / wide classes and the wide count, the cell map and the bucket hash -- and walk(), the candidate sets a
cell-walk over hashed buckets finds, which must be exactly the box-rule candidates."""
import numpy as np

import associate_ref as ar

MAX_DETECTIONS = 1 << 20
COORD_LIMIT = 2.0 ** 30
NONE, NARROW, WIDE = 0, 1, 2


def reach2(S, gate):
    """[n, 3]: (gate * S_aa) * (1 + 2^-10), plain multiplies in double"""
    diag = np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2]], axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        return (np.float64(gate) * diag) * np.float64(1.0 + 2.0 ** -10)


def narrow_limit2(cell):
    L = np.float64(cell) * np.float64(1.0 - 2.0 ** -20)
    with np.errstate(all="ignore"):
        lim2 = L * L
    return lim2 if np.finfo(np.float64).tiny <= lim2 <= np.finfo(np.float64).max else np.float64(-1.0)


def classes(zhat, r2, cell):
    """[n]: NONE for a NaN row, NARROW iff reach2 <= (cell (1 - 2^-20))^2 on all three axes, else WIDE"""
    lim2 = narrow_limit2(cell)
    with np.errstate(invalid="ignore"):
        narrow = (r2 <= lim2).all(axis=1)
    valid = ~np.isnan(np.asarray(zhat, dtype=np.float64)[:, 0])
    return np.where(valid, np.where(narrow, NARROW, WIDE), NONE)


def box(zhat, r2, det):
    """[n, M] bool: nu_a * nu_a <= reach2_a on every axis, nu the double d2 is formed from"""
    zhat = np.asarray(zhat, dtype=np.float64)
    z = np.asarray(det, dtype=np.float64)[:, 0:3]
    ok = np.ones((zhat.shape[0], z.shape[0]), dtype=bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            nu = z[None, :, a] - zhat[:, None, a]
            ok &= nu * nu <= r2[:, a][:, None]
    return ok


def cost(zhat, S, W, det, gate):
    """the cost matrix of the grid form: d2 in double where the box rule holds, NaN elsewhere; and reach2"""
    zhat, W = np.asarray(zhat, dtype=np.float64), np.asarray(W, dtype=np.float64)
    r2 = reach2(S, gate)
    D = ar.d2(zhat, W, det)
    return np.where(box(zhat, r2, det), D, np.nan), r2


def match(zhat, S, W, det, gate, rounds, cell):
    """the grid form's result: det_of_row, row_of_det, info = [matched, rounds_run, settled, wide], and the masked costs"""
    D, r2 = cost(zhat, S, W, det, gate)
    dr, rd, info = ar.match(D, gate, rounds)
    info[3] = int((classes(zhat, r2, cell) == WIDE).sum())
    return dr, rd, info, D


def coord(x, cell):
    """floor(x / cell) clamped to [-2^30, 2^30]; NaN -> -2^30"""
    with np.errstate(all="ignore"):
        q = np.floor(np.asarray(x, dtype=np.float64) / np.float64(cell))
    q = np.where(q >= -COORD_LIMIT, q, -COORD_LIMIT)
    q = np.where(q > COORD_LIMIT, COORD_LIMIT, q)
    return q.astype(np.int64)


def bucket(cx, cy, cz, H):
    """assoc_grid_hash: 32-bit arithmetic"""
    m = np.uint64(0xffffffff)
    u = lambda c: np.asarray(c, dtype=np.int64).astype(np.uint64) & m
    h = ((u(cx) * np.uint64(0x9E3779B1)) & m) ^ ((u(cy) * np.uint64(0x85EBCA77)) & m) ^ ((u(cz) * np.uint64(0xC2B2AE3D)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(13)
    return (h & np.uint64(H - 1)).astype(np.int64)


def plan_buckets(count, forced=0):
    if forced > 0:
        return forced
    h = 1024
    while h < 2 * count:
        h *= 2
    return h


def walk(zhat, r2, D, det, gate, cell, H_det, H_row):
    """What the device's walks visit.  Returns (by_row, by_det): for every row the set of detections its walk finds as candidates
    (a narrow row: the detection buckets of its 27 cells; a wide row: all detections), for every detection the set of rows (the row
    buckets of its 27 cells, then the wide list; a non-finite detection: nothing).  D: the UNMASKED d2; the box is tested here."""
    zhat = np.asarray(zhat, dtype=np.float64)
    z = np.asarray(det, dtype=np.float64)[:, 0:3]
    n, M = zhat.shape[0], z.shape[0]
    cls = classes(zhat, r2, cell)
    inbox = box(zhat, r2, det)
    with np.errstate(invalid="ignore"):
        cand = (D <= gate) & inbox
    finite = np.isfinite(z).all(axis=1)
    cd, cr = coord(z, cell), coord(zhat, cell)
    det_bk = {}
    for j in np.nonzero(finite)[0]:
        det_bk.setdefault(int(bucket(cd[j, 0], cd[j, 1], cd[j, 2], H_det)), []).append(int(j))
    row_bk = {}
    for i in np.nonzero(cls == NARROW)[0]:
        row_bk.setdefault(int(bucket(cr[i, 0], cr[i, 1], cr[i, 2], H_row)), []).append(int(i))
    wide = [int(i) for i in np.nonzero(cls == WIDE)[0]]
    nb = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    by_row = []
    for i in range(n):
        found = set()
        if cls[i] == NARROW:
            for dx, dy, dz in nb:
                for j in det_bk.get(int(bucket(cr[i, 0] + dx, cr[i, 1] + dy, cr[i, 2] + dz, H_det)), ()):
                    if cand[i, j]:
                        found.add(j)
        elif cls[i] == WIDE:
            found = set(int(j) for j in np.nonzero(cand[i])[0])
        by_row.append(found)
    by_det = []
    for j in range(M):
        found = set()
        if finite[j]:
            for dx, dy, dz in nb:
                for i in row_bk.get(int(bucket(cd[j, 0] + dx, cd[j, 1] + dy, cd[j, 2] + dz, H_row)), ()):
                    if cand[i, j]:
                        found.add(i)
            for i in wide:
                if cand[i, j]:
                    found.add(i)
        by_det.append(found)
    return by_row, by_det
