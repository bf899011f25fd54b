"""The NumPy twin of the duplicate-track search (tests/track_merge_ref.py) against things that call nothing of it: its rounds at
their fixed point against a plain-Python sorted greedy over pairs; the chain scene; the hashed 27-cell walk against the box-rule
candidates; the survivor order on all three levels of its key.  No GPU, no library."""
import numpy as np
import pytest

import associate_grid_ref as agr
import track_merge_ref as tm


def _greedy_pairs(D):
    """independent: every candidate pair (lo < hi) sorted by (d2, lo, hi), taken if both rows are free"""
    n = len(D)
    items = []
    for lo in range(n):
        for hi in range(lo + 1, n):
            v = D[lo][hi]
            if v == v:
                items.append((float(v), lo, hi))
    items.sort()
    partner = [-1] * n
    for _, lo, hi in items:
        if partner[lo] < 0 and partner[hi] < 0:
            partner[lo], partner[hi] = hi, lo
    return partner


def _sym(rng, n, levels, density):
    """a symmetric cost matrix with values from `levels` distinct costs (few levels: full of ties), NaN off the candidates"""
    A = rng.integers(0, levels, (n, n)).astype(np.float64) * 0.25
    A[rng.uniform(size=(n, n)) > density] = np.nan
    D = np.where(np.triu(np.ones((n, n), dtype=bool), 1), A, A.T)      # the upper triangle, mirrored
    np.fill_diagonal(D, np.nan)
    return D


def test_rounds_reach_sorted_greedy_over_pairs():
    rng = np.random.default_rng(0)
    tie_heavy = 0
    for k in range(400):
        n = int(rng.integers(0, 24))
        levels = 2 if k % 4 else 10 ** 6          # three in four: two cost levels only, everything ties
        tie_heavy += levels == 2
        D = _sym(rng, n, levels, float(rng.uniform(0.1, 1.0)))
        assert n == 0 or np.array_equal(np.isnan(D), np.isnan(D.T))
        partner, info = tm.match(D, 10 ** 6)
        assert list(partner) == _greedy_pairs(D.tolist()), k
        assert info[2] == 1 and info[0] == int((partner >= 0).sum()) // 2
        # a settled result is stable: fewer rounds give a subset of it
        p1, i1 = tm.match(D, 1)
        assert all(p1[i] in (-1, partner[i]) for i in range(n)) and (n == 0 or i1[1] == 1)
    assert tie_heavy >= 250


def _line(pos):
    z = np.zeros((len(pos), 3)); z[:, 0] = pos
    Sigma = np.tile(np.eye(3), (len(pos), 1, 1))
    return z, Sigma, np.ones(len(pos), dtype=bool)


@pytest.mark.parametrize("L", [2, 5, 8, 9])
def test_chain_scene_takes_one_pair_per_round(L):
    z, Sigma, valid = _line(tm.chain(L))
    hits = np.ones(L, dtype=np.uint8)
    gate, cell = float(L * L), 4.0 * L
    full = tm.find(z, Sigma, valid, hits, 0 * hits, gate, cell, 16, 1)
    assert full[3][3] == 0 and full[3][2] == 1
    need = full[3][1]
    assert need >= L // 2 and full[3][0] == L // 2          # (the count is the twin's; a last round may only confirm "settled")
    for rounds in range(1, need + 1):
        dup, partner, d2, info, D = tm.find(z, Sigma, valid, hits, 0 * hits, gate, cell, rounds, 1)
        assert info[0] == min(rounds, L // 2) and info[1] == rounds and info[2] == int(rounds >= need), (L, rounds, info)
    # pairs from the far end: (L-2, L-1), (L-4, L-3), ...
    assert [int(p) for p in full[1][L % 2:]] == [i + 1 if (i - L % 2) % 2 == 0 else i - 1 for i in range(L % 2, L)]


@pytest.mark.parametrize("scene", ["random", "borders", "negative"])
def test_hashed_walk_finds_exactly_the_box_rule_candidates(scene):
    rng = np.random.default_rng({"random": 1, "borders": 2, "negative": 3}[scene])
    n, cell, gate = 160, 1.0, 4.0
    if scene == "random":
        z = rng.uniform(0, 2.5, (n, 3))
    elif scene == "borders":
        z = rng.integers(0, 5, (n, 3)).astype(np.float64) * cell
        z[1::3] = np.nextafter(z[1::3], -np.inf); z[2::3] = np.nextafter(z[2::3], np.inf)
        z[n // 2:] += rng.integers(-1, 2, (n - n // 2, 3)) * 0.25
    else:
        z = rng.uniform(-2, 0.5, (n, 3)); z[::9] = -np.abs(z[::9]) - 1e9
    s = rng.uniform(0.002, 0.03, n)                                   # reach2 = 4 * 2 s (1 + 2^-10): narrow below s = 0.1249
    s[::7] = 0.2                                                      # wide
    Sigma = s[:, None, None] * np.eye(3)[None]
    valid = np.ones(n, dtype=bool); valid[5::31] = False
    hits = np.ones(n, dtype=np.uint8); hits[3::5] = 0
    cls = tm.classes(z, Sigma, valid, hits, 1, gate, cell)
    assert (cls == tm.WIDE).sum() > 0 and (cls == tm.NONE).sum() > 0 and (cls == tm.ELIGIBLE).sum() > n // 2
    D = tm.pairs(z, Sigma, cls, gate)
    want = [set(int(j) for j in np.nonzero(~np.isnan(D[i]))[0]) for i in range(n)]
    assert sum(len(w) for w in want) > 20
    for H in (agr.plan_buckets(n), 1, 4):
        assert tm.walk(z, cls, D, cell, H) == want, (scene, H)


def test_survivor_order_on_all_three_levels():
    partner = np.array([1, 0, 3, 2, 5, 4, -1])
    hits = np.array([3, 2, 4, 4, 7, 7, 9])
    miss = np.array([0, 0, 1, 2, 5, 5, 0])
    assert list(tm.weaker(partner, hits, miss)) == [0, 1, 0, 1, 0, 1, 0]      # fewer hits; more miss; the higher row
    # hits outrank miss
    assert list(tm.weaker(np.array([1, 0]), np.array([2, 3]), np.array([0, 200]))) == [1, 0]


def test_classes_and_retire_list():
    z, Sigma, valid = _line([0.0, 0.5, 10.0, 10.25, 20.0, 20.5, 30.0])
    Sigma = Sigma * 2.0 ** -7
    hits = np.array([5, 1, 2, 2, 0, 9, 3], dtype=np.uint8)
    miss = np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)
    dup, partner, d2, info, D = tm.find(z, Sigma, valid, hits, miss, 16.0, 2.0, 4, 1)
    assert list(partner) == [1, 0, 3, 2, -1, -1, -1] and list(dup) == [0, 1, 1, 0, 0, 0, 0] and info == [2, 1, 1, 0]
    assert d2[0] == d2[1] == 16.0 and d2[2] == d2[3] == 4.0 and d2[4] == -1.0      # d2 == gate: a candidate
    ids = [np.array([10, 11, 12], dtype=np.uint32), np.array([20, 21, 22, 23], dtype=np.uint32)]
    retired, kept, after = tm.retire(dup, partner, [3, 4], ids)
    assert list(retired) == [11, 12] and list(kept) == [10, 20]
    assert list(after[0]) == [10] and list(after[1]) == [20, 21, 22, 23]
    retired, kept, after = tm.retire(np.array([1, 0, 0, 0, 1, 0, 0]), np.array([1, 0, -1, -1, 5, 4, -1]), [3, 4], ids)
    assert list(retired) == [10, 21] and list(kept) == [11, 22] and list(after[0]) == [12, 11] and list(after[1]) == [20, 23, 22]
