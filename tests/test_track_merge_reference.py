"""The NumPy twin of the duplicate-track search (tests/track_merge_ref.py) against things that call nothing of it: its rounds at
their fixed point against a plain-Python sorted greedy over pairs; the chain scene; the hashed 27-cell walk against the box-rule
candidates; the survivor order on all three levels of its key; and its NUMBERS -- the row (zhat, Sigma) and the pair cost d2, in
float64 and float32 -- against the extended-precision reference tests/track_merge_highprec_ref.py (dense A P A^T + Q, Cholesky,
two triangular solves) on the coupled scenes of tests/track_merge_coupled_scenes.py, with the matching on the twin's costs held
to sorted greedy on the reference's.  No GPU, no library."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import associate_grid_ref as agr
import track_merge_coupled_scenes as cs
import track_merge_highprec_ref as hp
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


# ---------------------------------------------------------------------------------------------------------------- coupled scenes
# The twin's numbers against the extended-precision reference.  BOUND: 4 x the twin's own largest deviation over the three dt of a
# (model, precision), as measured with these scenes (profiles/track_merge_tolerances.txt): zhat in metres, Sigma relative to the
# row's largest word, d2 as |d2 - ref| / max(ref, 1) over the pairs with ref <= 4 gate.
COUPLED_DT = (2.0 ** -6, 0.01, 0.37)
COUPLED_N = {"f64": 96, "f32": 32}
COUPLED = [(name, dtype, dt) for name in hp.MODEL_NK for dtype in ("f64", "f32") for dt in COUPLED_DT]
BOUND = {
    ("uniform_velocity", "f64"): (4.1e-14, 1.1e-15, 2.5e-08),          # 4 x 1.02e-14, 2.77e-16, 6.16e-09
    ("uniform_velocity", "f32"): (9.2e-07, 5.0e-07, 3.5e-06),          # 4 x 2.29e-07, 1.26e-07, 8.63e-07
    ("uniform_acceleration", "f64"): (1.9e-14, 1.5e-15, 1.2e-08),      # 4 x 4.65e-15, 3.83e-16, 2.96e-09
    ("uniform_acceleration", "f32"): (1.7e-06, 6.3e-07, 5.2e-06),      # 4 x 4.20e-07, 1.57e-07, 1.31e-06
    ("angular_rates", "f64"): (4.7e-14, 1.5e-15, 8.1e-09),             # 4 x 1.17e-14, 3.69e-16, 2.02e-09
    ("angular_rates", "f32"): (1.5e-06, 7.6e-07, 3.9e-06),             # 4 x 3.78e-07, 1.91e-07, 9.66e-07
    ("angular_velocities", "f64"): (9.1e-15, 9.4e-16, 1.7e-08),        # 4 x 2.27e-15, 2.35e-16, 4.33e-09
    ("angular_velocities", "f32"): (9.2e-07, 3.9e-07, 7.7e-06),        # 4 x 2.29e-07, 9.79e-08, 1.92e-06
}


@functools.lru_cache(maxsize=None)
def _coupled(name, dtype, dt):
    """the first seed whose scene is separated (every d2 up to 4 gate from every other and from the gate, every box and class
    comparison from its limit, by more than 100 x the d2 allowance): the scene, the reference's numbers and the twin's"""
    T = cs.np_t(dtype)
    n = COUPLED_N[dtype]
    K = hp.MODEL_NK[name][1]
    cell = cs.CELL[dtype]
    hits, miss = cs.counters(n)
    for seed in range(12):
        s = cs.scene(name, dtype, n, seed, dt, third=(dtype == "f64"))
        zr, Sr, vr = hp.rows(s.x, s.P0, s.Q, dt, name)
        C, nu, d2r = hp.pairs(zr, Sr)
        zt, St, vt = tm.rows(s.x, s.P0, s.Q, np.zeros((K, K)), dt, name, T)
        d2t, inbox, ok = tm.pair_terms(zt, St, cs.GATE)
        dev = hp.deviation(d2t, d2r, 4 * cs.GATE)
        margins = hp.separation(zr, Sr, vr, cs.GATE, cell)
        if min(margins) > 100 * hp.allowance(dev):
            break
    else:
        raise AssertionError("no separated scene for %s %s dt %g" % (name, dtype, dt))
    Dr, cls = hp.decide(zr, Sr, vr, hits, cs.MIN_HITS, cs.GATE, cell)
    return SimpleNamespace(s=s, seed=seed, n=n, cell=cell, hits=hits, miss=miss, zr=zr, Sr=Sr, vr=vr, C=C, d2r=d2r, zt=zt, St=St, vt=vt,
                           d2t=d2t, dev=dev, Dr=Dr, cls=cls)


@pytest.mark.parametrize("name,dtype,dt", COUPLED)
def test_coupled_scene_is_coupled(name, dtype, dt):
    """what the scene claims: every cross-axis block of P and Q populated, the acceleration state non-zero, twins, classes"""
    c = _coupled(name, dtype, dt)
    s = c.s
    N, K = hp.MODEL_NK[name]
    for r in range(3):
        for q in range(3):
            for i in range(N // K):
                for j in range(N // K):
                    assert (s.P0[:, r + i * K, q + j * K] != 0).all() and s.Q[r + i * K, q + j * K] != 0
    assert (s.x[:, K:K + 3] != 0).any(axis=1).all() and (np.linalg.eigvalsh(s.P0) > 0).all() and np.linalg.eigvalsh(s.Q)[0] > 0
    if N // K == 3:
        assert (s.x[:, 2 * K:2 * K + 3] != 0).all()
    up = np.triu(np.ones((c.n, c.n), dtype=bool), 1)
    cand = up & ~np.isnan(c.Dr)
    twins = sum(bool(cand[k - 1, k]) for k in range(1, c.n, 4))
    assert twins >= c.n // 16 and (c.cls == hp.WIDE).any() and (c.vr & (c.hits < cs.MIN_HITS)).any()
    assert (cs.correlation(c.C.astype(np.float64))[cand] >= 0.3).sum() * 3 >= cand.sum()


@pytest.mark.parametrize("name,dtype,dt", COUPLED)
def test_coupled_twin_rows_and_costs_against_the_reference(name, dtype, dt):
    c = _coupled(name, dtype, dt)
    L = np.longdouble
    z = float(np.abs(c.zt.astype(L) - c.zr).max())
    S = float((np.abs(c.St.astype(L) - c.Sr).max(axis=(1, 2)) / np.abs(c.Sr).max(axis=(1, 2))).max())
    print("twin %s %s dt %g seed %d: zhat %.3e m, Sigma %.3e, d2 %.3e" % (name, dtype, dt, c.seed, z, S, c.dev))
    bz, bS, bd = BOUND[(name, dtype)]
    assert z <= bz and S <= bS and c.dev <= bd
    assert c.vt.all() and c.vr.all()
    # the twin's cost exists exactly where the reference factorises C
    d2t, inbox, ok = tm.pair_terms(c.zt, c.St, cs.GATE)
    up = np.triu(np.ones((c.n, c.n), dtype=bool), 1)
    assert np.array_equal(ok[up], ~np.isnan(c.d2r.astype(np.float64))[up])


@pytest.mark.parametrize("name,dtype,dt", COUPLED)
def test_coupled_matching_is_sorted_greedy_on_the_reference_costs(name, dtype, dt):
    c = _coupled(name, dtype, dt)
    dup, partner, d2, info, D = tm.find(c.zt, c.St, c.vt, c.hits, c.miss, cs.GATE, c.cell, 16, cs.MIN_HITS)
    assert np.array_equal(np.isnan(D), np.isnan(c.Dr))                         # the same candidates, pair for pair
    want = hp.greedy(c.Dr)
    assert np.array_equal(partner, want) and info[2] == 1 and info[0] == int((want >= 0).sum()) // 2 > 0
    assert info[3] == int((c.cls == hp.WIDE).sum()) and np.array_equal(tm.classes(c.zt, c.St, c.vt, c.hits, cs.MIN_HITS, cs.GATE, c.cell), c.cls)
    m = partner >= 0
    err = np.abs(d2[m].astype(np.longdouble) - c.d2r[np.nonzero(m)[0], partner[m]]) / np.maximum(c.d2r[np.nonzero(m)[0], partner[m]], 1)
    assert float(err.max()) <= c.dev


def test_coupled_scenes_spread_of_conditioning():
    """f64: at least 10 candidate pairs with cond(C) >= 1e4 in every scene's family of three dt, some near 1e6; f32: cond(C) <= 1e2"""
    for name in hp.MODEL_NK:
        high, near = 0, 0
        for dt in COUPLED_DT:
            c = _coupled(name, "f64", dt)
            up = np.triu(np.ones((c.n, c.n), dtype=bool), 1)
            k = hp.cond(c.C)[up & ~np.isnan(c.Dr)]
            high += int((k >= 1e4).sum()); near += int(((k >= 2.5e5) & (k <= 4e6)).sum())
            assert (k >= 1e4).sum() >= 10 and (k < 1e2).sum() >= 5, (name, dt)
            c = _coupled(name, "f32", dt)
            up = np.triu(np.ones((c.n, c.n), dtype=bool), 1)
            e = c.cls == hp.ELIGIBLE
            assert hp.cond(c.C)[up & e[:, None] & e[None, :]].max() <= 1e2, (name, dt)
        assert high >= 30 and near >= 9, (name, high, near)


def test_reference_pieces_against_closed_forms():
    """the reference itself on cases with known answers: A(dt) of each model on a state, a diagonal C, a C that does not factorise"""
    x = np.arange(1.0, 19.0)
    for name, (N, K) in hp.MODEL_NK.items():
        z, S, v = hp.rows(x[None, :N], np.eye(N)[None], np.zeros((N, N)), 0.5, name)
        want = x[0:3] + 0.5 * x[K:K + 3] + (0.125 * x[2 * K:2 * K + 3] if N // K == 3 else 0.0)
        assert np.array_equal(z[0].astype(np.float64), want) and v[0]
        s = 1.0 + 0.25 + (1.0 / 64 if N // K == 3 else 0.0)
        assert np.array_equal(S[0].astype(np.float64), s * np.eye(3))
    z = np.array([[0.0, 0, 0], [1.0, 2.0, 3.0]])
    Sg = np.stack([np.diag([0.5, 1.0, 2.0])] * 2)
    C, nu, d2 = hp.pairs(z, Sg)
    assert float(d2[0, 1]) == float(d2[1, 0]) == 1.0 + 2.0 + 2.25 and np.isnan(float(d2[0, 0]))
    bad = Sg.copy(); bad[0, 0, 1] = bad[0, 1, 0] = 3.0
    assert np.isnan(hp.pairs(z, bad)[2].astype(np.float64)).all()
    assert list(hp.greedy(np.array([[np.nan, 2.0, 1.0], [2.0, np.nan, 1.0], [1.0, 1.0, np.nan]]))) == [2, -1, 0]
