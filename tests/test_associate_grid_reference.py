"""CPU-only: the NumPy twin of the grid form (tests/associate_grid_ref.py) against itself -- a cell-walk over hashed buckets finds
exactly the box-rule candidates, for every row and every detection, on random and tie-heavy scenes, with planned and tiny bucket
counts and with positions snapped to cell borders; the box contains the gate for well-conditioned S; the wide count; and the
masked cost matrix through associate_ref.match gives the plain form's result where the box loses no pair."""
import numpy as np
import pytest

import associate_grid_ref as agr
import associate_ref as ar


def _scene(rng, n, M, cell, spread, snap=False, ties=False, scale_every=7):
    """n targets with S = 0.0025 A A^T + 0.01 I (every scale_every-th 64 x that: wide), M detections near them and elsewhere"""
    zhat = rng.uniform(-spread, spread, (n, 3))
    det = np.concatenate([zhat[rng.integers(0, n, M - M // 4)] + rng.normal(0, 0.2, (M - M // 4, 3)), rng.uniform(-spread, spread, (M // 4, 3))])
    if ties:                           # a coarse lattice: many equal offsets, many equal d2
        zhat, det = np.round(zhat * 4) / 4, np.round(det * 4) / 4
    if snap:                           # onto cell borders, and one ulp either side
        zhat[::2] = np.round(zhat[::2] / cell) * cell
        det[::2] = np.round(det[::2] / cell) * cell
        zhat[1::4] = np.nextafter(np.round(zhat[1::4] / cell) * cell, -np.inf)
        det[1::4] = np.nextafter(np.round(det[1::4] / cell) * cell, np.inf)
    S = np.empty((n, 3, 3))
    for i in range(n):
        A = np.eye(3) if ties else rng.normal(size=(3, 3))
        S[i] = 0.0025 * (A @ A.T) + 0.01 * np.eye(3)
        if i % scale_every == 0:
            S[i] *= 64.0
    W, valid = ar.invert(S)
    assert valid.all()
    d = np.zeros((M, 7)); d[:, :3] = det; d[:, 6] = 1.0
    return zhat, S, W, d


@pytest.mark.parametrize("snap,ties", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("H", [None, 1, 4])
def test_cell_walk_finds_exactly_the_box_rule_candidates(snap, ties, H):
    rng = np.random.default_rng(11 + 2 * snap + ties)
    gate = 9.0
    for cell, spread in ((0.5, 3.0), (1.0, 6.0), (0.37, 3.0)):
        n, M = 90, 160
        zhat, S, W, det = _scene(rng, n, M, cell, spread, snap, ties)
        det[5, 0] = np.nan; det[6, 1] = np.inf; det[7, 2] = -np.inf
        D = ar.d2(zhat, W, det)
        Dm, r2 = agr.cost(zhat, S, W, det, gate)
        cls = agr.classes(zhat, r2, cell)
        assert (cls == agr.NARROW).any() and (cls == agr.WIDE).any()
        Hd, Hr = (agr.plan_buckets(M), agr.plan_buckets(n)) if H is None else (H, H)
        by_row, by_det = agr.walk(zhat, r2, D, det, gate, cell, Hd, Hr)
        with np.errstate(invalid="ignore"):
            cand = Dm <= gate
        assert cand.sum() > n // 2
        for i in range(n):
            assert by_row[i] == set(np.nonzero(cand[i])[0].tolist()), (cell, i, cls[i])
        for j in range(M):
            assert by_det[j] == set(np.nonzero(cand[:, j])[0].tolist()), (cell, j)


def test_box_contains_the_gate_and_the_masked_match_is_the_plain_match():
    rng = np.random.default_rng(3)
    gate = 9.0
    zhat, S, W, det = _scene(rng, 130, 257, 0.5, 4.0)
    D = ar.d2(zhat, W, det)
    Dm, r2 = agr.cost(zhat, S, W, det, gate)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(D <= gate, Dm <= gate)                      # a well-conditioned S: the box loses nothing
    for rounds in (1, 3, 16):
        dr, rd, info, _ = agr.match(zhat, S, W, det, gate, rounds, 0.5)
        pr, pd, pinfo = ar.match(D, gate, rounds)
        assert np.array_equal(dr, pr) and np.array_equal(rd, pd) and info[:3] == pinfo[:3]
        assert info[3] == int((agr.classes(zhat, r2, 0.5) == agr.WIDE).sum()) and 0 < info[3] < 130


def test_classes_and_the_cell_map():
    zhat = np.array([[0.0, 0, 0], [np.nan, 0, 0], [1.0, 1, 1], [2.0, 2, 2]])
    r2 = np.array([[0.2, 0.2, 0.2], [0.2, 0.2, 0.2], [0.2, 0.3, 0.2], [np.nan, 0.1, 0.1]])
    lim2 = agr.narrow_limit2(0.5)
    assert lim2 == (0.5 * (1 - 2.0 ** -20)) ** 2 and 0.2 <= lim2 < 0.25 < 0.3
    assert list(agr.classes(zhat, r2, 0.5)) == [agr.NARROW, agr.NONE, agr.WIDE, agr.WIDE]
    assert agr.narrow_limit2(1e-200) == -1.0 and agr.narrow_limit2(1e200) == -1.0       # no slot is narrow: every valid slot wide
    assert list(agr.classes(zhat, r2, 1e200)) == [agr.WIDE, agr.NONE, agr.WIDE, agr.WIDE]
    c = agr.coord(np.array([-0.0, -1e-300, 0.49999, 0.5, -0.5, -0.50001, 1e300, -1e300, np.nan, np.inf, -np.inf, 2.0 ** 29, 2.0 ** 29 + 0.5]), 0.5)
    assert list(c) == [0, -1, 0, 1, -1, -2, 2 ** 30, -2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30, 2 ** 30, 2 ** 30]
    assert agr.plan_buckets(0) == 1024 and agr.plan_buckets(512) == 1024 and agr.plan_buckets(513) == 2048 and agr.plan_buckets(10 ** 6) == 2 ** 21
    assert agr.plan_buckets(10 ** 6, 4) == 4
    b = agr.bucket(np.arange(-50, 50), np.arange(-50, 50)[::-1], np.arange(100) - 7, 1024)
    assert b.min() >= 0 and b.max() < 1024 and len(set(b.tolist())) > 80
    assert (agr.bucket(np.arange(10), 0, 0, 1) == 0).all()
