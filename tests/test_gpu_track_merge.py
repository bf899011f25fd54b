"""Duplicate tracks on the device (target_manager_find_duplicates_dev, target_manager_retire_duplicates) against the
NumPy twin tests/track_merge_ref.py.

EXACTLY THE TWIN.  The scenes are test_gpu_associate[_grid]'s worlds: fresh targets whose state is known on the CPU, positions and
velocities on a binary grid and dt = 2^-6, so that the twin in the batch's precision forms the very doubles the table kernel forms
(zhat, Sigma); the pair's C, its inverse, d2 and the box are then plain double arithmetic in one fixed order on both sides: every
output array and info is compared bit for bit, no tolerance anywhere.  Counters are raised beforehand with lifecycle calls on
hand-built masks.  Every seventh P0 is 64 x the others' (wide at the cell used), every fifth target has fewer hits than min_hits,
planted twins sit at small binary offsets; planned buckets and TE_ASSOC_GRID_BUCKETS = 1 and 4 must give the same bytes.
The shared-axes batch with flagged uniform tiles has been stepped: its x and P are read back, and the twin's row from them is still
exact (the table multiplies by powers of two only), so it is held to the twin bit for bit like every other case."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import associate_ref as ar
import track_merge_ref as tm
from test_gpu_associate import DT, World, _bits, _cuda, _np_t
from test_gpu_associate_grid import _init, _scaled_world

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

GATE = 9.0
CELL = 0.5            # reach = sqrt(9 (1 + 2^-10) 2 Sigma_aa): about 0.42 m for the plain rows, 3.4 m for the scaled ones
MIN_HITS = 2
BUCKETS = (None, 1, 4)
NS = [0, 1, 2, 8, 9, 63, 64, 65, 130, 257, 300]


def _counters(n):
    """every fifth target below MIN_HITS; the others 2 .. 4 hits; some misses"""
    i = np.arange(n)
    hits = np.where(i % 5 == 0, 1, 2 + i % 3).astype(np.uint8)
    miss = ((i // 3) % 3).astype(np.uint8)
    return hits, miss


def _raise_counters(mgr, per_batch):
    """per_batch: [(hits, miss)] per batch in batches() order: hits calls with a 1 first, then miss calls with a 0"""
    top_h = max([int(h.max()) for h, m in per_batch if len(h)] + [0])
    top_m = max([int(m.max()) for h, m in per_batch if len(m)] + [0])
    total = top_h + top_m
    for k in range(total):
        masks = []
        for h, m in per_batch:      # a target's last m calls are misses, the h calls before them hits, anything earlier a miss
            assert (h >= 1).all()
            last_hit = total - m.astype(np.int64)
            on = (last_hit - h.astype(np.int64) <= k) & (k < last_hit)
            masks.append(_cuda(on.astype(np.uint8), np.uint8) if len(h) else torch.zeros(1, dtype=torch.uint8, device="cuda"))
        mgr.lifecycle(None, SimpleNamespace(has_meas=masks), max_misses=0, birth_type=None, first_id=0, t_birth=0.0, dt0=DT)
    for b, (h, m) in zip(mgr.batches(), per_batch):
        got_m, got_h = b.track_counts()
        assert np.array_equal(got_h, h) and np.array_equal(got_m, m)


def _twin_world(name, dtype, layout, n, seed):
    """the scaled world with twins planted: every fourth target (1 mod 4) sits at a small binary offset from its predecessor and
    moves with it; offsets from 2^-5 to 0.6 m, so that some twins fall outside the gate"""
    w = _scaled_world(name, dtype, layout, n, seed)
    rng = np.random.default_rng(77 + seed)
    for i in range(1, n, 4):
        off = np.zeros(3)
        off[rng.integers(0, 3)] = (1 + (i // 4) % 19) * 2.0 ** -5
        off[rng.integers(0, 3)] += 2.0 ** -6 * rng.integers(-2, 3)
        w.p0[i, :3] = w.p0[i - 1, :3] + off
        w.v0[i] = w.v0[i - 1]
    for i in range(2, n, 8):                   # ... and a third track next to some twins: the first then waits for a second round
        w.p0[i, :3] = w.p0[i - 1, :3] + [0.0, 2.0 ** -6, 2.0 ** -7]
        w.v0[i] = w.v0[i - 1]
    return w


def _twin_rows(w, dt=DT):
    x, P = w.cpu_state()
    T = _np_t(w.dtype)
    Q = w.Q[w.cls] if w.cls is not None else w.Q
    R = w.R[w.cls] if w.cls is not None else w.R
    Q, R = Q.astype(T).astype(np.float64), R.astype(T).astype(np.float64)
    return tm.rows(x.astype(T).astype(np.float64), P.astype(T).astype(np.float64), Q, R, dt, w.name, T)


def _arrays(r, sizes):
    torch.cuda.synchronize()
    cat = lambda ts: np.concatenate([t.cpu().numpy()[:n] for t, n in zip(ts, sizes)] + [np.zeros(0, dtype=ts[0].cpu().numpy().dtype if ts else np.uint8)])
    return [cat(r.dup), cat(r.partner_batch), cat(r.partner_slot), cat(r.d2), r.info.cpu().numpy().copy()]


def _same_bytes(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)


def _want(rows, hits, miss, gate, cell, rounds, min_hits, sizes):
    """the twin's arrays in the device's form: partner rows translated to (batch, slot)"""
    zhat, Sigma, valid = rows
    dup, partner, d2, info, D = tm.find(zhat, Sigma, valid, hits, miss, gate, cell, rounds, min_hits)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pb = np.where(partner >= 0, np.searchsorted(off, np.maximum(partner, 0), side="right") - 1, -1).astype(np.int32)
    ps = np.where(partner >= 0, partner - off[np.maximum(pb, 0)], -1).astype(np.int32)
    return [dup, pb, ps, d2, np.array(info, dtype=np.int32)], partner, D


def _check(got, want, what):
    assert list(got[4]) == list(want[4]), (what, got[4], want[4])
    for k in range(3):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(_bits(got[3]), _bits(want[3])), what


def _run_case(name, dtype, layout, n, seed=0, rounds_list=(1, 16)):
    res = {}
    hits, miss = _counters(n)
    for buckets in BUCKETS:
        w = _twin_world(name, dtype, layout, n, seed)
        rows = _twin_rows(w)
        what = "%s %s %s n %d buckets %s" % (name, dtype, layout, n, buckets)
        if buckets is None and n >= 63:        # the scene is not vacuous: known before the device is touched
            want, partner, D = _want(rows, hits, miss, GATE, CELL, 16, MIN_HITS, [n])
            cls = tm.classes(rows[0], rows[1], rows[2], hits, MIN_HITS, GATE, CELL)
            d2, inbox, ok = tm.pair_terms(rows[0], rows[1], GATE)
            e = cls == tm.ELIGIBLE
            with np.errstate(invalid="ignore"):
                lost = ok & e[:, None] & e[None, :] & (d2 <= 4 * GATE) & ~(inbox & (d2 <= GATE))
            assert 0 < want[4][0] and 0 < want[4][3] < n, what
            assert (rows[2] & (hits < MIN_HITS)).any() and lost.any() and (e & (partner < 0)).any(), what
        b = _init(w, buckets)
        if b is None:
            r = w.mgr.find_duplicates(DT, GATE, CELL, rounds=4, min_hits=MIN_HITS)
            torch.cuda.synchronize()
            assert list(r.info.cpu().numpy()) == [0, 0, 1, 0], what
            w.mgr.close()
            continue
        _raise_counters(w.mgr, [(hits, miss)])
        for rounds in rounds_list:
            r = w.mgr.find_duplicates(DT, GATE, CELL, rounds=rounds, min_hits=MIN_HITS)
            got = _arrays(r, [n])
            _check(got, _want(rows, hits, miss, GATE, CELL, rounds, MIN_HITS, [n])[0], what + " rounds %d" % rounds)
            res[(buckets, rounds)] = got
        w.mgr.close()
    for rounds in rounds_list:
        for buckets in BUCKETS[1:]:
            if (buckets, rounds) in res:
                _same_bytes(res[(None, rounds)], res[(buckets, rounds)], (name, n, rounds, buckets))


# ---------------------------------------------------------------------------------------------------------------- 1. exactly the twin
@pytest.mark.parametrize("n", NS)
def test_exactly_the_twin(n):
    _run_case("uniform_velocity", "f64", "301", n)


@pytest.mark.parametrize("name,dtype,layout", [("uniform_acceleration", "f64", "301"), ("angular_rates", "f64", "301"),
                                                ("angular_velocities", "f64", "301"), ("uniform_velocity", "f32", "301"),
                                                ("uniform_velocity", "f64", "201"), ("angular_rates", "f64", "full"),
                                                ("uniform_acceleration", "f64", "full"), ("angular_velocities", "f32", "packed"),
                                                ("uniform_velocity", "f64", "packed"), ("angular_rates", "f64", "classes"),
                                                ("uniform_acceleration", "f64", "301shared")])
def test_exactly_the_twin_models_precisions_layouts(name, dtype, layout):
    _run_case(name, dtype, layout, 130, seed=1)


def test_shared_axes_batch_with_flagged_uniform_tiles():
    """Sigma must come from the tile's block: with a cell between the reach of the current Sigma and the reach the stale per-slot
    words (P0) would give, no row is wide, where stale words would make every row wide.  The filters have been stepped, so x and P
    are read back; the row is still the twin's bit for bit, because every product the table forms is with dt = 2^-6 or dt^2 / 2 --
    exact, fused or not -- and the sums are taken in the kernel's order."""
    name, n = "uniform_acceleration", 130
    w = World(name, "f64", "301shared", n, seed=7)
    for i in range(1, n, 4):
        w.p0[i, :3] = w.p0[i - 1, :3] + [2.0 ** -4, 0.0, 0.0]
        w.v0[i] = w.v0[i - 1]
    b = _init(w)
    ticks = 4
    meas = np.zeros((ticks, n, 7)); meas[:, :, 6] = 1.0
    for s in range(ticks):
        meas[s, :, :3] = w.p0[:, :3] + w.v0[:, :3] * DT * (s + 1)
    b.step_sequence(DT, _cuda(meas.transpose(0, 2, 1), np.float64), use_graph=True)
    assert b.shared_axes == 1 and b.uniform_tiles > 0
    hits = np.full(n, 1, dtype=np.uint8)
    _raise_counters(w.mgr, [(hits, 0 * hits)])
    x, P = w.mgr.get_state_batch(w.ids)
    rows = tm.rows(x, P, w.Q, w.R, DT, name)
    x0, P0 = w.cpu_state()
    stale = tm.rows(x0, P0, w.Q, w.R, DT, name)
    r_now = 2.0 * GATE * np.stack([rows[1][:, a, a] for a in range(3)], 1).max() * (1 + 2.0 ** -10)
    r_stale = 2.0 * GATE * np.stack([stale[1][:, a, a] for a in range(3)], 1).min() * (1 + 2.0 ** -10)
    assert r_stale > 1.5 * r_now
    cell = float(np.sqrt(0.5 * (r_now * 1.2 + r_stale / 1.2)))
    want, partner, D = _want(rows, hits, 0 * hits, GATE, cell, 16, 1, [n])
    assert want[4][3] == 0 and want[4][0] >= n // 4 - 1
    assert (tm.classes(stale[0], stale[1], stale[2], hits, 1, GATE, cell) == tm.WIDE).all()
    got = _arrays(w.mgr.find_duplicates(DT, GATE, cell, rounds=16, min_hits=1), [n])
    _check(got, want, "uniform tiles")                           # every array and info by bits, d2 included
    assert b.shared_axes == 1 and b.uniform_tiles > 0
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- 2. edge cases
def _half_world(pos, name="uniform_velocity", mgr=None, ids=None):
    """targets at `pos` with Sigma = I / 2 exactly at dt = 0 (P0 = Q = R = I / 4): C = I and d2 = |nu|^2 for every pair"""
    w = World(name, "f64", "301", len(pos), seed=0, mgr=mgr, ids=ids)
    N, K = ar.MODEL_NK[name]
    w.Q, w.R, w.P0 = 0.25 * np.eye(N), 0.25 * np.eye(K), 0.25 * np.eye(N)
    w.p0[:, :3] = pos
    w.v0[:] = 0.0
    return w


def _edge(pos, gate, cell, rounds=16, hits=None, miss=None, min_hits=0):
    """half-worlds at pos for planned buckets, 1 and 4 against the twin; returns the arrays"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    hits = np.zeros(n, dtype=np.uint8) if hits is None else np.asarray(hits, dtype=np.uint8)
    miss = np.zeros(n, dtype=np.uint8) if miss is None else np.asarray(miss, dtype=np.uint8)
    rows = (pos.copy(), np.tile(0.5 * np.eye(3), (n, 1, 1)), np.ones(n, dtype=bool))
    want = _want(rows, hits, miss, gate, cell, rounds, min_hits, [n])[0]
    out = None
    for buckets in BUCKETS:
        w = _half_world(pos)
        _init(w, buckets)
        if hits.any() or miss.any():
            _raise_counters(w.mgr, [(hits, miss)])
        got = _arrays(w.mgr.find_duplicates(0.0, gate, cell, rounds=rounds, min_hits=min_hits), [n])
        _check(got, want, "edge buckets %s" % buckets)
        if out is not None:
            _same_bytes(out, got, "edge buckets")
        out = got
        w.mgr.close()
    return out


def test_planted_exact_ties():
    # two equidistant partners: row 1 picks the lower row; the third row is left over
    out = _edge([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]], gate=4.0, cell=2.5)
    assert list(out[2]) == [1, 0, -1] and list(out[0]) == [0, 1, 0] and list(out[4]) == [1, 2, 1, 0]
    # the same tie across buckets (cell 2.5: 9 -> 3, 10 and 11 -> 4); equal hits and miss: the higher row is the duplicate
    out = _edge([[11.0, 0, 0], [10.0, 0, 0], [9.0, 0, 0]], gate=4.0, cell=2.5, hits=[2, 2, 2], miss=[1, 1, 1])
    assert list(out[2]) == [1, 0, -1] and list(out[0]) == [0, 1, 0]
    # fewer hits lose, whatever the row; at equal hits more miss lose
    out = _edge([[0.0, 0, 0], [1.0, 0, 0], [10.0, 0, 0], [11.0, 0, 0]], gate=4.0, cell=2.5, hits=[1, 2, 3, 3], miss=[0, 1, 1, 0])
    assert list(out[0]) == [1, 0, 1, 0] and _bits(out[3]).tolist() == _bits(np.ones(4)).tolist()


def test_d2_equal_to_the_gate_is_a_candidate():
    pos = [[0.0, 0, 0], [3.0, 4.0, 0], [100.0, 0, 0], [103.0, 4.0, 0]]
    out = _edge(pos, gate=25.0, cell=6.0)
    assert list(out[2]) == [1, 0, 3, 2] and _bits(out[3]).tolist() == _bits(np.full(4, 25.0)).tolist() and list(out[4]) == [2, 1, 1, 0]
    out = _edge(pos, gate=float(np.nextafter(25.0, 0.0)), cell=6.0)
    assert list(out[2]) == [-1] * 4 and list(out[4]) == [0, 1, 1, 0]


@pytest.mark.parametrize("L", [7, 8])
def test_chain_scene_rounds(L):
    pos = np.stack([tm.chain(L), np.zeros(L), np.zeros(L)], axis=1)
    rows = (pos, np.tile(0.5 * np.eye(3), (L, 1, 1)), np.ones(L, dtype=bool))
    z = np.zeros(L, dtype=np.uint8)
    need = tm.find(rows[0], rows[1], rows[2], z, z, float(L * L), 4.0 * L, 16, 0)[3][1]      # the count is the twin's
    assert L // 2 <= need <= L // 2 + 1
    for rounds in (1, 2, L // 2, L // 2 + 1):
        out = _edge(pos, gate=float(L * L), cell=4.0 * L, rounds=rounds)
        assert list(out[4]) == [min(rounds, L // 2), min(rounds, need), int(rounds >= need), 0]


def test_one_cell_borders_negative_and_large_coordinates():
    rng = np.random.default_rng(6)
    cell = 2.5
    k = rng.integers(-6, 6, (40, 3)).astype(np.float64)
    pos = k * cell
    pos[1::3] = np.nextafter(pos[1::3], -np.inf)
    pos[2::3] = np.nextafter(pos[2::3], np.inf)
    pos = np.concatenate([pos, k * cell + rng.integers(-1, 2, (40, 3)) * 1.0])
    out = _edge(pos, gate=2.0, cell=cell)
    assert out[4][0] > 5 and out[4][3] == 0
    one = _edge(np.abs(pos), gate=2.0, cell=1e6)                   # everything in one cell
    assert one[4][0] > 5
    base = np.concatenate([rng.uniform(-40, 40, (30, 3)), rng.uniform(-1, 1, (30, 3)) * 8 + [1e9, -1e9, 1e9]])
    base = np.round(base * 16) / 16
    pos = np.concatenate([base, base[::2] + np.round(rng.normal(0, 0.25, base[::2].shape) * 64) / 64])
    out = _edge(pos, gate=0.75, cell=1.25)
    assert out[4][0] > 10 and out[4][3] == 0
    wide = _edge(pos, gate=0.75, cell=0.5)                         # reach 0.87 > cell: every row wide, excluded
    assert list(wide[4]) == [0, 1, 1, len(pos)]


def test_an_indefinite_pair_sum_and_a_nan_state():
    nan = float("nan")
    mgr = te.TargetManager(dtype="f64", lanes_per_target=3)
    N = 6
    Q, R, P0 = 0.25 * np.eye(N), 4.0 * np.eye(3), 0.5 * np.eye(N)
    bad = P0.copy(); bad[0, 1] = bad[1, 0] = 2.0                  # Sigma indefinite, S = Sigma + 4 I positive definite: a valid row
    p0 = np.zeros((5, 7)); p0[:, 6] = 1.0
    p0[:, 0] = [0.0, 0.5, 1.0, 50.0, nan]
    assert mgr.init_batch(np.arange(5, dtype=np.uint32) + 5, DT, 0.0, p0, np.zeros((5, 6)), np.zeros((5, 6)),
                          type=te.MODEL_TYPES["uniform_velocity"], Q=Q, R=R, P0=np.stack([bad, P0, P0, P0, P0])) == 5
    x = np.zeros((5, N)); x[:, 0] = p0[:, 0]
    rows = tm.rows(x, np.stack([bad, P0, P0, P0, P0]), Q, R, 0.0, "uniform_velocity")
    assert rows[2][:4].all() and not rows[2][4]
    z = np.zeros(5, dtype=np.uint8)
    want, partner, D = _want(rows, z, z, 9.0, 8.0, 16, 0, [5])
    assert list(partner) == [-1, 2, 1, -1, -1]                   # row 0's pair sums do not invert; the NaN row is invalid
    got = _arrays(mgr.find_duplicates(0.0, 9.0, 8.0, rounds=16, min_hits=0), [5])
    _check(got, want, "indefinite")
    mgr.close()


def _mixed(buckets=None):
    os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)
    if buckets is not None:
        os.environ["TE_ASSOC_GRID_BUCKETS"] = str(buckets)
    try:
        mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
    finally:
        os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    w1 = _half_world(np.array([[0.0, 0, 0], [19.0, 0, 0], [30.0, 0, 0]]), name="angular_rates", mgr=mgr, ids=np.array([1, 2, 3], dtype=np.uint32))
    w2 = _half_world(np.array([[20.0, 0, 0], [40.0, 0, 0], [31.0, 0, 0], [41.0, 0, 0]]), name="angular_velocities", mgr=mgr,
                     ids=np.array([11, 12, 13, 14], dtype=np.uint32))
    w1.init(); w2.init()
    ws = {te.MODEL_TYPES[w.name]: w for w in (w1, w2)}
    return mgr, [ws[b.type] for b in mgr.batches()]


def test_mixed_manager_with_cross_batch_pairs_and_refusals():
    res = None
    for buckets in BUCKETS:
        mgr, ws = _mixed(buckets)
        sizes = [w.n for w in ws]
        pos = np.concatenate([w.p0[:, :3] for w in ws])
        n = len(pos)
        rows = (pos, np.tile(0.5 * np.eye(3), (n, 1, 1)), np.ones(n, dtype=bool))
        z = np.zeros(n, dtype=np.uint8)
        want, partner, D = _want(rows, z, z, 4.0, 2.5, 16, 0, sizes)
        assert (want[1][want[1] >= 0] != np.repeat(np.arange(2), sizes)[want[1] >= 0]).sum() == 4      # two cross-batch pairs
        got = _arrays(mgr.find_duplicates(0.0, 4.0, 2.5, rounds=16, min_hits=0), sizes)
        _check(got, want, "mixed")
        if res is not None:
            _same_bytes(res, got, "mixed buckets")
        res = got
        mgr.close()
    # several shards, populated with twins: refused, and size, ids, slot tables, counters, rejection runs, x and P stay byte for byte
    sh = te.TargetManager(dtype="f64", devices=[0, 0], lanes_per_target=301)
    w = _half_world(np.array([[0.0, 0, 0], [0.5, 0, 0], [10.0, 0, 0], [10.5, 0, 0], [20.0, 0, 0], [20.5, 0, 0]]), mgr=sh,
                    ids=np.arange(6, dtype=np.uint32) + 40)
    assert sh.init_batch(w.ids, DT, 0.0, w.p0, w.v0, w.a0, type=te.MODEL_TYPES[w.name], Q=w.Q, R=w.R, P0=w.P0) == 6
    assert sh.size() == 6 and len(sh.batches()) >= 2             # (the ids are dealt to both shards)
    before = _snapshot(sh)
    with pytest.raises(RuntimeError, match="shards"):
        sh.find_duplicates(0.0, 4.0, 2.5, min_hits=0)
    assert _snapshot(sh) == before
    with pytest.raises(RuntimeError, match="shards"):
        sh.retire_duplicates(0.0, 4.0, 2.5, min_hits=0)
    assert _snapshot(sh) == before and sh.size() == 6
    sh.close()


def test_two_calls_and_a_captured_graph_give_the_same_bytes():
    n = 300
    hits, miss = _counters(n)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = _twin_world("angular_rates", "f64", "301", n, seed=9)
        _init(w, 4)
        _raise_counters(w.mgr, [(hits, miss)])
        r = w.mgr.find_duplicates(DT, GATE, CELL, rounds=3, min_hits=MIN_HITS)
        stream.synchronize()
        first = _arrays(r, [n])
        _check(first, _want(_twin_rows(w), hits, miss, GATE, CELL, 3, MIN_HITS, [n])[0], "first")
        _same_bytes(first, _arrays(w.mgr.find_duplicates(DT, GATE, CELL, rounds=3, min_hits=MIN_HITS), [n]), "repeat")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            w.mgr.find_duplicates(DT, GATE, CELL, rounds=3, min_hits=MIN_HITS, out=r)
        for _ in range(2):
            for t in r.dup + r.partner_batch + r.partner_slot + r.d2 + [r.info]:
                t.fill_(7)
            g.replay()
            stream.synchronize()
            _same_bytes(first, _arrays(r, [n]), "replay")
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- 3. retire
def _snapshot(m):
    bs = m.batches()
    ids = m.getAvailableTargets()
    x, P = m.get_state_batch(ids) if len(ids) else (np.zeros(0), np.zeros(0))
    return (m.size(), ids.tobytes(), [b.slot_ids().tobytes() for b in bs], [tuple(c.tobytes() for c in b.track_counts()) for b in bs],
            [b.rejection_runs().tobytes() for b in bs], x.tobytes(), P.tobytes())


def _retire_world(mgr=None):
    """130 scaled targets with planted twins, the last three a chain A-B-C (one pair per call: the second call finds the next)"""
    n = 130
    w = _twin_world("uniform_velocity", "f64", "301", n, seed=3)
    w.p0[-3:, :3] = [50.0, 50.0, 50.0] + np.stack([tm.chain(3) * 2.0 ** -5, np.zeros(3), np.zeros(3)], axis=1)
    w.v0[-3:] = 0.0
    w.P0[-3:] = w.P0[1]
    return w


def test_retire_duplicates_against_the_host_composed_path():
    hits, miss = _counters(130)
    hits[-3:], miss[-3:] = 3, 0
    wa, wb = _retire_world(), _retire_world()
    _init(wa); _init(wb)
    for w in (wa, wb):
        _raise_counters(w.mgr, [(hits, miss)])
    A, B = wa.mgr, wb.mgr
    rows = _twin_rows(wa)
    dup, partner, d2, info, D = tm.find(rows[0], rows[1], rows[2], hits, miss, GATE, CELL, 16, MIN_HITS)
    retired, kept, after = tm.retire(dup, partner, [130], [wa.ids])
    assert len(retired) == info[0] > 5 and partner[-1] == 128 and partner[-3] == -1         # the chain: its last two only
    assert (np.nonzero(dup)[0] < 130 - len(retired)).any()                                   # a survivor is moved into a hole
    # refusals first: nothing changes
    before = _snapshot(A)
    from target_estimation_amd import capi
    lib = A._lib
    ids_out = (C.c_uint * 200)()
    info4 = (C.c_long * 4)()
    up = lambda a: C.cast(a, capi.c_uint_p)
    assert lib.target_manager_retire_duplicates(A._h, DT, GATE, 16, CELL, MIN_HITS, up(ids_out), up(ids_out), len(retired) - 1, info4) == -1
    assert "targets to retire" in capi.last_error() and _snapshot(A) == before
    per = (capi.DupOut * 2)()
    dev = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.target_manager_find_duplicates_dev(A._h, DT, GATE, 16, CELL, MIN_HITS, per, 2, dev.data_ptr()) == -1
    assert "is not the manager's" in capi.last_error()
    assert lib.target_manager_find_duplicates_dev(A._h, DT, GATE, 16, CELL, MIN_HITS, per, 1, dev.data_ptr()) == -1
    assert "dup_out_dev of a non-empty batch is NULL" in capi.last_error()
    torch.cuda.synchronize()
    assert _snapshot(A) == before and not dev.cpu().numpy().any()
    # the call against the host-composed path
    out = A.retire_duplicates(DT, GATE, CELL, rounds=16, min_hits=MIN_HITS)
    assert B.erase_batch(retired) == len(retired)
    assert np.array_equal(out.retired_ids, retired) and np.array_equal(out.kept_ids, kept)
    assert [out.retired, out.rounds_run, out.settled, out.wide] == [info[0], info[1], info[2], info[3]]
    assert np.array_equal(A.batches()[0].slot_ids(), after[0])
    assert _snapshot(A) == _snapshot(B)
    left_h, left_m = lr_erase(hits, dup), lr_erase(miss, dup)
    got_m, got_h = A.batches()[0].track_counts()
    assert np.array_equal(got_h, left_h) and np.array_equal(got_m, left_m)
    # a step, then the cleaned population: the chain's next pair
    n2 = A.size()
    x, _ = A.get_state_batch(A.batches()[0].slot_ids())
    meas = np.zeros((7, n2)); meas[6] = 1.0; meas[:3] = x[:, :3].T
    for m in (A, B):
        m.batches()[0].step(DT, _cuda(meas, np.float64), torch.ones(n2, dtype=torch.uint8, device="cuda"))
    assert _snapshot(A) == _snapshot(B)
    out2 = A.retire_duplicates(DT, GATE, CELL, rounds=16, min_hits=MIN_HITS)
    chain_ids = set(int(i) for i in wa.ids[-3:])
    assert len(set(int(i) for i in out2.retired_ids) & chain_ids) == 1 and A.size() == n2 - out2.retired
    A.close(); B.close()


def lr_erase(col, dup):
    import lifecycle_ref as lr
    return lr.erase([np.asarray(col)], np.nonzero(dup)[0])[0]
