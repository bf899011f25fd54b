"""NumPy twin of the duplicate-track search (csrc/track_merge_plan.hpp, csrc/track_merge.hip).

rows(): zhat and validity from associate_ref.table with the class's R, Sigma from the same table with R = 0.  classes(): none /
eligible / wide.  pairs(): the symmetric cost matrix of eligible rows with the gate and the pair box applied (NaN: no candidate).
match(): the rounds of mutual best, exactly the device's rule.  weaker(): the survivor rule.  find(): all of it, what
target_manager_find_duplicates_dev writes.  retire(): the per-batch retire list and the layout lifecycle_ref.erase leaves.
walk(): the candidates a hashed 27-cell walk finds.  chain(): the scene that matches one pair per round."""
import numpy as np

import associate_grid_ref as agr
import associate_ref as ar
import lifecycle_ref as lr

NONE, ELIGIBLE, WIDE = 0, 1, 2


def rows(x, P, Q, R, dt, name, T=np.float64):
    """zhat [n, 3] (NaN: invalid), Sigma [n, 3, 3], valid [n]: the association's row valid AND Sigma's six words finite"""
    zhat, S, W, valid = ar.table(x, P, Q, R, dt, name, T)
    _, Sigma, _, _ = ar.table(x, P, Q, np.zeros_like(np.asarray(R, dtype=np.float64)), dt, name, T)
    Sigma = np.asarray(Sigma, dtype=np.float64)
    valid = valid & np.isfinite(Sigma).all(axis=(1, 2))
    zhat = np.asarray(zhat, dtype=np.float64).copy()
    valid = valid & ~np.isnan(zhat[:, 0])                                # (a NaN state: the device tests the row's first word)
    return zhat, Sigma, valid


def classes(zhat, Sigma, valid, hits, min_hits, gate, cell):
    """[n]: NONE (invalid, or hits < min_hits), ELIGIBLE (narrow by reach2(gate, 2 Sigma_aa)), WIDE"""
    r2 = agr.reach2(2.0 * np.asarray(Sigma, dtype=np.float64), gate)
    lim2 = agr.narrow_limit2(cell)
    with np.errstate(invalid="ignore"):
        narrow = (r2 <= lim2).all(axis=1)
    ok = np.asarray(valid, dtype=bool) & ~np.isnan(np.asarray(zhat)[:, 0]) & (np.asarray(hits).astype(np.int64) >= int(min_hits))
    return np.where(ok, np.where(narrow, ELIGIBLE, WIDE), NONE)


def pair_terms(zhat, Sigma, gate):
    """for every ordered pair lo < hi (mirrored to hi, lo): d2 [n, n], inbox [n, n], invertible [n, n]; the diagonal is NaN / False"""
    zhat, Sigma = np.asarray(zhat, dtype=np.float64), np.asarray(Sigma, dtype=np.float64)
    n = zhat.shape[0]
    if n == 0:
        return np.zeros((0, 0)), np.zeros((0, 0), dtype=bool), np.zeros((0, 0), dtype=bool)
    with np.errstate(all="ignore"):
        C = Sigma[:, None, :, :] + Sigma[None, :, :, :]                  # fl(a + b) == fl(b + a): the order of the sum is immaterial
        V, ok = ar.invert(C.reshape(n * n, 3, 3))
        V, ok = V.reshape(n, n, 3, 3), ok.reshape(n, n)
        nu = zhat[None, :, :] - zhat[:, None, :]                         # [i, j] = z_j - z_i: for i < j this is z_hi - z_lo
        nx, ny, nz = nu[..., 0], nu[..., 1], nu[..., 2]
        t0 = (V[..., 0, 0] * nx + V[..., 0, 1] * ny) + V[..., 0, 2] * nz
        t1 = (V[..., 0, 1] * nx + V[..., 1, 1] * ny) + V[..., 1, 2] * nz
        t2 = (V[..., 0, 2] * nx + V[..., 1, 2] * ny) + V[..., 2, 2] * nz
        d2 = (nx * t0 + ny * t1) + nz * t2
        one = np.float64(1.0 + 2.0 ** -10)
        inbox = np.ones((n, n), dtype=bool)
        for a in range(3):
            inbox &= nu[..., a] * nu[..., a] <= (np.float64(gate) * C[..., a, a]) * one
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    d2 = np.where(up, d2, d2.T)                                          # the (lo, hi) value on both sides
    inbox = np.where(up, inbox, inbox.T)
    ok = np.where(up, ok, ok.T)
    np.fill_diagonal(d2, np.nan); np.fill_diagonal(inbox, False); np.fill_diagonal(ok, False)
    return d2, inbox, ok


def pairs(zhat, Sigma, cls, gate):
    """the cost matrix: d2 where both rows are eligible, C inverts, d2 <= gate and the pair box holds; NaN elsewhere"""
    d2, inbox, ok = pair_terms(zhat, Sigma, gate)
    e = np.asarray(cls) == ELIGIBLE
    with np.errstate(invalid="ignore"):
        cand = ok & inbox & (d2 <= gate) & e[:, None] & e[None, :]
    return np.where(cand, d2, np.nan)


def match(D, rounds):
    """The device's rounds on the symmetric cost matrix D (NaN: no candidate).  partner [n], info = [pairs, rounds_run, settled]."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    partner = np.full(n, -1, dtype=np.int64)
    cand = ~np.isnan(D)
    n_pairs, run, settled = 0, 0, int(n == 0)
    for _ in range(rounds):
        if settled:
            break
        free = cand & (partner < 0)[:, None] & (partner < 0)[None, :]
        pick = ar._pick(D, free, 1)
        open_ = 0
        new = partner.copy()
        for i in range(n):
            if partner[i] >= 0 or pick[i] < 0:
                continue
            j = pick[i]
            if pick[j] == i:
                new[i] = j
                n_pairs += int(i < j)
            else:
                open_ += 1
        partner = new
        run += 1
        settled = int(open_ == 0)
    return partner, [n_pairs, run, settled]


def weaker(partner, hits, miss):
    """dup [n] uint8: of a matched pair the weaker row: fewer hits; at equal hits more miss; at equal both the higher row"""
    partner = np.asarray(partner)
    hits, miss = np.asarray(hits).astype(np.int64), np.asarray(miss).astype(np.int64)
    n = len(partner)
    dup = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        j = partner[i]
        if j < 0:
            continue
        if hits[i] != hits[j]:
            w = hits[i] < hits[j]
        elif miss[i] != miss[j]:
            w = miss[i] > miss[j]
        else:
            w = i > j
        dup[i] = int(w)
    return dup


def find(zhat, Sigma, valid, hits, miss, gate, cell, rounds, min_hits):
    """what find_duplicates writes, over the concatenated rows: dup, partner (row, -1), d2 (-1.0: none), info [4], and D"""
    cls = classes(zhat, Sigma, valid, hits, min_hits, gate, cell)
    D = pairs(zhat, Sigma, cls, gate)
    partner, info = match(D, rounds)
    n = len(partner)
    d2 = np.where(partner >= 0, D[np.arange(n), np.maximum(partner, 0)], -1.0) if n else np.zeros(0)
    return weaker(partner, hits, miss), partner, d2, info + [int((cls == WIDE).sum())], D


def retire(dup, partner, sizes, ids):
    """sizes / ids per batch (rows concatenated in batch order).  Returns (retired ids, kept ids, the ids of every batch afterwards):
    per batch in batch order, ascending former slot; the layout is lifecycle_ref.erase's."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = np.concatenate([np.asarray(i, dtype=np.uint32) for i in ids]) if len(ids) else np.zeros(0, dtype=np.uint32)
    retired, kept, after = [], [], []
    for b, n in enumerate(sizes):
        slots = np.nonzero(np.asarray(dup[off[b]:off[b + 1]]))[0]
        retired.extend(int(flat[off[b] + s]) for s in slots)
        kept.extend(int(flat[partner[off[b] + s]]) for s in slots)
        after.append(lr.erase([np.asarray(ids[b], dtype=np.uint32)], slots)[0])
    return np.array(retired, dtype=np.uint32), np.array(kept, dtype=np.uint32), after


def walk(zhat, cls, D, cell, H):
    """for every eligible row the set of candidates its walk over the 27 hashed row buckets around its cell finds (never itself)"""
    zhat = np.asarray(zhat, dtype=np.float64)
    n = zhat.shape[0]
    c = agr.coord(zhat, cell)
    bk = {}
    for i in np.nonzero(np.asarray(cls) == ELIGIBLE)[0]:
        bk.setdefault(int(agr.bucket(c[i, 0], c[i, 1], c[i, 2], H)), []).append(int(i))
    nb = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    out = []
    for i in range(n):
        found = set()
        if cls[i] == ELIGIBLE:
            for dx, dy, dz in nb:
                for j in bk.get(int(agr.bucket(c[i, 0] + dx, c[i, 1] + dy, c[i, 2] + dz, H)), ()):
                    if j != i and not np.isnan(D[i, j]):
                        found.add(j)
        out.append(found)
    return out


def chain(L):
    """L points on the x axis with strictly decreasing integer gaps L, L - 1, ..., 2: with equal Sigma and a wide gate every point's
    nearest neighbour is the next one, so only the last two are mutual; one pair per round, from the far end"""
    gaps = np.arange(L, 1, -1, dtype=np.float64)
    return np.concatenate([[0.0], np.cumsum(gaps)])
