"""The NumPy twin of the association (tests/associate_ref.py) against what it claims: rounds of mutual best reach sorted greedy
global-nearest-neighbour, also on cost matrices full of ties; the chain scene matches one pair per round; the table's float64 form
stays near its longdouble form."""
import numpy as np
import pytest

import associate_ref as ar


@pytest.mark.parametrize("seed", range(40))
def test_rounds_reach_sorted_greedy_on_random_costs(seed):
    rng = np.random.default_rng(seed)
    n, M = int(rng.integers(0, 14)), int(rng.integers(0, 14))
    D = rng.uniform(0.0, 10.0, (n, M))
    D[rng.uniform(size=D.shape) < 0.1] = np.nan
    gate = float(rng.choice([2.0, 6.0, np.inf]))
    dr, rd, info = ar.match(D, gate, ar.MAX_ROUNDS)
    gr, gd = ar.greedy(D, gate)
    assert info[2] == 1
    assert np.array_equal(dr, gr) and np.array_equal(rd, gd)
    assert info[0] == int((dr >= 0).sum())


@pytest.mark.parametrize("seed", range(300))
def test_rounds_reach_sorted_greedy_on_tie_heavy_costs(seed):
    rng = np.random.default_rng(1000 + seed)
    n, M = int(rng.integers(1, 10)), int(rng.integers(1, 10))
    D = rng.integers(0, 4, (n, M)).astype(np.float64)       # four values only: ties everywhere
    gate = float(rng.choice([1.0, 2.0, np.inf]))
    dr, rd, info = ar.match(D, gate, ar.MAX_ROUNDS)
    gr, gd = ar.greedy(D, gate)
    assert info[2] == 1, "min(n, M) <= 9 pairs are matched in at most 9 rounds"
    assert np.array_equal(dr, gr) and np.array_equal(rd, gd)


def test_fewer_rounds_are_a_prefix_of_the_greedy_result():
    rng = np.random.default_rng(5)
    D = rng.integers(0, 6, (12, 12)).astype(np.float64)
    full, _, _ = ar.match(D, np.inf, ar.MAX_ROUNDS)
    last = 0
    for r in range(1, 8):
        dr, rd, info = ar.match(D, np.inf, r)
        got = dr >= 0
        assert np.array_equal(dr[got], full[got])           # what is matched is what greedy matches
        assert info[0] >= last and info[1] <= r
        last = info[0]
        if info[2]:
            assert np.array_equal(dr, full)


@pytest.mark.parametrize("L", [1, 2, 6, 9])
def test_chain_matches_one_pair_per_round(L):
    t, d = ar.chain(L)
    D = (d[None, :] - t[:, None]) ** 2
    assert len(set(np.round(D.ravel(), 9))) >= 2 * L - 1
    for rounds in range(1, L + 2):
        dr, rd, info = ar.match(D, np.inf, rounds)
        assert info[0] == min(rounds, L)
        assert info[1] == min(rounds, L)
        assert info[2] == int(rounds >= L)
        want = np.full(L, -1)
        want[L - min(rounds, L):] = np.arange(L - min(rounds, L), L)     # from the far end
        assert np.array_equal(dr, want) and np.array_equal(rd, want)


def test_empty_sides():
    for shape in [(0, 0), (0, 5), (5, 0)]:
        dr, rd, info = ar.match(np.zeros(shape), 1.0, 4)
        assert info == [0, 0, 1, 0] and (dr == -1).all() and (rd == -1).all()
    dr, rd, info = ar.match(np.full((3, 3), 5.0), 1.0, 4)     # nobody has a candidate: one round finds that out
    assert info == [0, 1, 1, 0]


def test_nan_and_gate_are_rejections():
    D = np.array([[1.0, np.nan], [np.nan, 4.0]])
    dr, rd, info = ar.match(D, 4.0, 4)
    assert list(dr) == [0, 1] and info[0] == 2
    dr, rd, info = ar.match(D, np.nextafter(4.0, 0.0), 4)
    assert list(dr) == [0, -1] and info[0] == 1


@pytest.mark.parametrize("name", list(ar.MODEL_NK))
def test_table_float64_near_longdouble_and_validity(name):
    N, K = ar.MODEL_NK[name]
    rng = np.random.default_rng(N)
    n = 40
    x = rng.uniform(-3, 3, (n, N))
    A = rng.normal(size=(n, N, N)) * 0.05
    P = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(N)
    Q = 1e-6 * np.eye(N)
    R = 2.5e-3 * np.eye(K)
    z64, S64, W64, ok64 = ar.table(x, P, Q, R, 0.02, name, np.float64)
    zl, Sl, Wl, okl = ar.table(x, P, Q, R, 0.02, name, np.longdouble)
    assert ok64.all() and okl.all()
    assert np.abs(S64 - Sl).max() <= 1e-14 * np.abs(Sl).max()
    for k in range(n):
        assert np.allclose((W64[k] @ S64[k]).astype(np.float64), np.eye(3), atol=1e-9)
    det = np.concatenate([z64 + rng.normal(0, 0.05, (n, 3)), np.zeros((n, 4))], axis=1)
    D64, Dl = ar.d2(z64, W64, det), ar.d2(zl, Wl, det)
    assert (D64.diagonal() >= 0).all()
    assert np.abs(D64 - Dl).max() <= 1e-9 * np.maximum(Dl, 1).max()
    # the validity rule: a non-finite S, a non-positive diagonal entry, a non-positive determinant
    bad = np.stack([np.diag([1.0, -1.0, 1.0]), np.diag([1.0, 0.0, 1.0]), np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]]),
                    np.diag([np.inf, 1.0, 1.0]), np.diag([np.nan, 1.0, 1.0]), np.eye(3)])
    W, valid = ar.invert(bad)
    assert list(valid) == [False] * 5 + [True]
    assert np.isnan(W[:5]).all() and np.array_equal(W[5], np.eye(3))
