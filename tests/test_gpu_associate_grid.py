"""The grid form of the association on the device (target_batch_associate_grid[_dev], target_manager_associate_grid[_dev];
DESIGN 3.19) against the NumPy twin tests/associate_grid_ref.py and against the brute-force device form.

EXACTLY THE TWIN.  The scenes are test_gpu_associate's worlds: fresh targets whose state is known on the CPU, positions and
velocities on a binary grid and dt = 2^-6, so that every product with dt is exact and the twin in the batch's precision forms the
very doubles the table kernel forms (zhat, S, W).  d2 and the box are then plain double arithmetic in one fixed order on both
sides: every output array is compared bit for bit, no tolerance anywhere.  The P0 of every seventh target is 64 x the others', so
that with the cell used some slots are narrow and some wide; planned buckets and TE_ASSOC_GRID_BUCKETS = 1 and 4 must give the
same bytes.
EQUAL TO THE BRUTE-FORCE FORM wherever the box loses no pair: asserted on the CPU first, for every scene."""
import os

import numpy as np
import pytest

import associate_grid_ref as agr
import associate_ref as ar
from test_gpu_associate import DT, World, _bits, _cuda, _dets, _labelled, _np_t, _planted, _unit_world

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

GATE = 9.0
CELL = 0.5            # reach = sqrt(9 (1 + 2^-10) S_aa): about 0.34 .. 0.43 m for the plain slots, 2.4 m and more for the scaled ones
BUCKETS = (None, 1, 4)
NS = [0, 1, 63, 64, 65, 130, 300]
MS = [0, 1, 67, 257, 300]


def _init(w, buckets=None):
    """the manager (TE_ASSOC_GRID_BUCKETS is read when it is created) and the targets; returns the batch"""
    if buckets is not None:
        os.environ["TE_ASSOC_GRID_BUCKETS"] = str(buckets)
    try:
        return w.init()
    finally:
        os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)


def _scaled_world(name, dtype, layout, n, seed, mgr=None, ids=None):
    """a World whose every seventh target has 64 x the P0 (a class of its own in the "classes" layout): wide at CELL"""
    w = World(name, dtype, layout, n, seed, mgr=mgr, ids=ids)
    N, _ = ar.MODEL_NK[name]
    if layout == "classes":
        w.cls = (np.arange(n) % 7 == 0).astype(np.uint32)
        w.P0 = np.stack([w.P0[0], 64.0 * w.P0[1]])
    else:
        P0 = np.broadcast_to(w.P0, (n, N, N)).copy()
        P0[::7] *= 64.0
        w.P0 = P0 if n > 0 else w.P0
    return w


def _twin_tables(w, dt=DT):
    x, P = w.cpu_state()
    tl, ts = w.tables(x, P, dt)
    return tl, tuple(np.asarray(t, dtype=np.float64) for t in ts[:3])


def _arrays(r):
    ts = [r.meas, r.has_meas, r.det_of_slot, r.d2_of_slot, r.slot_of_det, r.d2_of_det, r.info]
    return [t.cpu().numpy().copy() for t in ts]


def _check_twin(w, r, det, ts, gate, rounds, cell, what):
    """every output against the twin, bit for bit; returns info"""
    n, M = w.n, det.shape[0]
    zhat, S, W = ts
    dr, rd, info, D = agr.match(zhat, S, W, det, gate, rounds, cell)
    torch.cuda.synchronize()
    got_info = list(r.info.cpu().numpy())
    assert got_info == info, (what, got_info, info)
    dos, sod = r.det_of_slot.cpu().numpy()[:n], r.slot_of_det.cpu().numpy()
    d2s, d2d = r.d2_of_slot.cpu().numpy()[:n], r.d2_of_det.cpu().numpy()
    assert np.array_equal(dos, dr) and np.array_equal(sod, rd), what
    want_s = np.where(dr >= 0, D[np.arange(n), np.maximum(dr, 0)], -1.0) if M else np.full(n, -1.0)
    want_d = np.where(rd >= 0, D[np.maximum(rd, 0), np.arange(M)], -1.0) if n else np.full(M, -1.0)
    assert np.array_equal(_bits(d2s), _bits(want_s)) and np.array_equal(_bits(d2d), _bits(want_d)), what
    T = _np_t(w.dtype)
    got = dr >= 0
    meas, has = r.meas.cpu().numpy()[:, :n], r.has_meas.cpu().numpy()[:n]
    want = np.tile(np.array([0, 0, 0, 0, 0, 0, 1], dtype=T)[:, None], (1, n))
    want[:, got] = det[dr[got]].T.astype(T)
    assert meas.dtype == T and np.array_equal(meas.view(np.uint8), want.view(np.uint8)), what
    assert np.array_equal(has, got.astype(np.uint8)), what
    return info


def _same_bytes(a, b, what, skip_wide=False):
    for k, (x, y) in enumerate(zip(a, b)):
        if skip_wide and k == len(a) - 1:
            x, y = x[:3], y[:3]
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)


def _run_case(name, dtype, layout, n, M, seed=0, rounds_list=(1, 16)):
    res = {}
    for buckets in BUCKETS:
        w = _scaled_world(name, dtype, layout, n, seed)
        tl, ts = _twin_tables(w)
        det = _planted(w, tl, M, seed)
        b = _init(w, buckets)
        what = "%s %s %s n %d M %d buckets %s" % (name, dtype, layout, n, M, buckets)
        if b is None:     # no target at all: through the manager
            r = w.mgr.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=4, cell=CELL)
            torch.cuda.synchronize()
            assert list(r.info.cpu().numpy()) == [0, 0, 1, 0] and (r.slot_of_det.cpu().numpy() == -1).all(), what
            w.mgr.close()
            continue
        for rounds in rounds_list:
            r = b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=rounds, cell=CELL)
            info = _check_twin(w, r, det, ts, GATE, rounds, CELL, what + " rounds %d" % rounds)
            res[(buckets, rounds)] = _arrays(r)
        if n >= 63 and M >= 67:
            assert 0 < info[3] < n and 0 < info[0] < min(n, M), (what, info)       # narrow and wide slots, unmatched on both sides
        w.mgr.close()
    for rounds in rounds_list:
        for buckets in BUCKETS[1:]:
            if (buckets, rounds) in res:
                _same_bytes(res[(None, rounds)], res[(buckets, rounds)], (name, n, M, rounds, buckets))


# ---------------------------------------------------------------------------------------------------------------- 1. exactly the twin
@pytest.mark.parametrize("n", NS)
def test_exactly_the_twin(n):
    for M in MS:
        _run_case("uniform_velocity", "f64", "301", n, M)


@pytest.mark.parametrize("name,dtype,layout", [("uniform_acceleration", "f64", "301"), ("angular_rates", "f64", "301"),
                                                ("angular_velocities", "f64", "301"), ("uniform_velocity", "f32", "301"),
                                                ("uniform_velocity", "f64", "201"), ("angular_rates", "f64", "full"),
                                                ("uniform_acceleration", "f64", "full"), ("angular_velocities", "f32", "packed"),
                                                ("uniform_velocity", "f64", "packed"), ("angular_rates", "f64", "classes")])
def test_exactly_the_twin_models_precisions_layouts(name, dtype, layout):
    _run_case(name, dtype, layout, 130, 257)


def test_shared_axes_batch_with_flagged_uniform_tiles():
    """A shared-axes batch after a recorded sequence holds flagged uniform tiles: S's diagonal must come from the tile's block, as
    the table row does.  The filters have been stepped, so the state is the device's: the grid form is held to the brute-force form
    byte for byte, and the wide count to the twin's -- with a cell between the reach of the current S and the reach that the stale
    per-slot words (P0) would give: 0 wide slots, where stale words would make every slot wide."""
    name, n = "uniform_acceleration", 130
    w = World(name, "f64", "301shared", n, seed=7)
    b = _init(w)
    rng = np.random.default_rng(3)
    ticks = 4
    meas = np.zeros((ticks, n, 7)); meas[:, :, 6] = 1.0
    for s in range(ticks):
        meas[s, :, :3] = w.p0[:, :3] + w.v0[:, :3] * DT * (s + 1) + rng.normal(0, 0.02, (n, 3))
    b.step_sequence(DT, _cuda(meas.transpose(0, 2, 1), np.float64), use_graph=True)
    assert b.shared_axes == 1 and b.uniform_tiles > 0
    x, P = w.mgr.get_state_batch(w.ids)
    tl, ts = w.tables(x, P, DT)
    zhat, S, W = (np.asarray(t, dtype=np.float64) for t in ts[:3])
    x0, P0 = w.cpu_state()
    stale = w.tables(x0, P0, DT)[1]
    r_now, r_stale = agr.reach2(S, GATE), agr.reach2(np.asarray(stale[1], dtype=np.float64), GATE)
    assert r_stale.min() > 1.5 * r_now.max()                     # ... known before the call
    cell = float(np.sqrt(0.5 * (r_now.max() * 1.2 + r_stale.min() / 1.2)))
    assert (agr.classes(zhat, r_now, cell) == agr.NARROW).all() and (agr.classes(zhat, r_stale, cell) == agr.WIDE).all()
    det = np.zeros((n, 7)); det[:, 6] = 1.0
    det[:, :3] = zhat + rng.normal(0, 0.05, (n, 3))
    det = det[rng.permutation(n)]
    D, _ = agr.cost(zhat, S, W, det, GATE)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(D <= GATE, ar.d2(zhat, W, det) <= GATE)
    rb = _arrays(b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=16))
    rg = _arrays(b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=16, cell=cell))
    torch.cuda.synchronize()
    _same_bytes(rb, rg, "uniform tiles", skip_wide=True)
    assert rg[-1][0] > n // 2 and rg[-1][3] == 0, rg[-1]
    assert b.shared_axes == 1 and b.uniform_tiles > 0
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the brute-force form
def _correlated_world(n, seed, buckets=None):
    """uniform_velocity f64 in the full layout with S = 0.0025 A A^T + (0.01 + P0_vv dt^2 + Q) I per target, A random; every fifth
    target's A has singular values 30, 1, 1/30 in a random frame: an axis ratio of 10^6 in A A^T"""
    w = World("uniform_velocity", "f64", "full", n, seed)
    rng = np.random.default_rng(1000 + seed)
    N = 6
    w.Q, w.R = 1e-6 * np.eye(N), 0.01 * np.eye(3)
    P0 = np.tile(1e-2 * np.eye(N), (max(n, 1), 1, 1))
    for i in range(n):
        A = rng.normal(size=(3, 3))
        if i % 5 == 4:
            U, _, Vt = np.linalg.svd(A)
            A = U @ np.diag([30.0, 1.0, 1.0 / 30.0]) @ Vt
        P0[i, :3, :3] = 0.0025 * (A @ A.T)
        P0[i, :3, :3] = 0.5 * (P0[i, :3, :3] + P0[i, :3, :3].T)
    w.P0 = P0[:n] if n else w.P0
    return w


@pytest.mark.parametrize("n", NS[1:])
def test_equal_to_the_brute_force_form(n):
    for M in MS[1:]:
        w = _correlated_world(n, seed=n + M)
        tl, ts = _twin_tables(w)
        zhat, S, W = ts
        det = _planted(w, tl, M, n + M)
        D, _ = agr.cost(zhat, S, W, det, GATE)
        with np.errstate(invalid="ignore"):
            plain, boxed = ar.d2(zhat, W, det) <= GATE, D <= GATE
        assert np.array_equal(plain, boxed), (n, M, int((plain & ~boxed).sum()))      # the box loses no pair: known before the call
        b = _init(w)
        for rounds in (1, 16):
            rb = _arrays(b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=rounds))
            r = b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=rounds, cell=CELL)
            _check_twin(w, r, det, ts, GATE, rounds, CELL, "correlated n %d M %d rounds %d" % (n, M, rounds))
            _same_bytes(rb, _arrays(r), (n, M, rounds), skip_wide=True)
            assert rb[-1][3] == 0
        w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- 3. edge cases
def _edge(pos_t, pos_d, gate, cell, rounds=16, brute=True):
    """targets with S = I exactly (dt = 0) at pos_t, detections at pos_d: the grid form for planned buckets, 1 and 4 against the
    twin and (brute) the brute-force form; returns the arrays and info"""
    pos_t, det = np.asarray(pos_t, dtype=np.float64), _dets(np.asarray(pos_d, dtype=np.float64))
    n = len(pos_t)
    S = np.tile(np.eye(3), (n, 1, 1))
    out = None
    for buckets in BUCKETS:
        w = _unit_world(pos_t)
        b = _init(w, buckets)
        r = b.associate(_cuda(det, np.float64), 0.0, gate=gate, rounds=rounds, cell=cell)
        _check_twin(w, r, det, (pos_t, S, S), gate, rounds, cell, "edge buckets %s" % buckets)
        got = _arrays(r)
        if brute:
            _same_bytes(_arrays(b.associate(_cuda(det, np.float64), 0.0, gate=gate, rounds=rounds)), got, "edge brute", skip_wide=True)
        if out is not None:
            _same_bytes(out, got, "edge buckets")
        out = got
        w.mgr.close()
    return out


def test_positions_on_cell_borders():
    cell = 2.5
    rng = np.random.default_rng(5)
    k = rng.integers(-6, 6, (40, 3)).astype(np.float64)
    pos_t = k * cell                                                      # exactly on borders
    pos_t[1::3] = np.nextafter(pos_t[1::3], -np.inf)
    pos_t[2::3] = np.nextafter(pos_t[2::3], np.inf)
    off = rng.integers(-1, 2, (40, 3)) * 2.0                              # offsets of exactly 0 or +-2 per axis: d2 in {0, 4, 8, 12}
    pos_d = np.concatenate([k * cell + off, (k + rng.integers(-1, 2, (40, 3))) * cell])
    out = _edge(pos_t, pos_d, gate=4.0, cell=cell)
    assert out[-1][3] == 0 and out[-1][0] > 0
    out = _edge(pos_t, pos_d, gate=12.0, cell=cell)                       # reach 3.47 > cell: every slot wide
    assert out[-1][3] == 40


def test_negative_and_large_coordinates_with_a_unit_cell():
    rng = np.random.default_rng(6)
    base_t = np.concatenate([rng.uniform(-40, 40, (30, 3)), rng.uniform(-1, 1, (30, 3)) * 8 + [1e9, -1e9, 1e9],
                             rng.uniform(-1, 1, (10, 3)) * 8 + [-2.0 ** 31, 2.0 ** 31, 0.0]])
    base_t = np.round(base_t * 16) / 16
    pos_d = base_t + np.round(rng.normal(0, 0.25, base_t.shape) * 64) / 64
    pos_d = np.concatenate([pos_d, -base_t[:20]])
    out = _edge(base_t, pos_d[rng.permutation(len(pos_d))], gate=0.75, cell=1.0)
    assert out[-1][3] == 0 and out[-1][0] > 20


def test_nan_and_inf_detections_and_an_indefinite_s():
    nan, inf = float("nan"), float("inf")
    mgr = te.TargetManager(dtype="f64", lanes_per_target=3)
    N = 6
    Q, R, P0 = 0.25 * np.eye(N), 0.25 * np.eye(3), 0.5 * np.eye(N)
    bad = P0.copy(); bad[0, 1] = bad[1, 0] = 2.0
    p0 = np.zeros((3, 7)); p0[:, 6] = 1.0; p0[:, 0] = [0.0, 100.0, 200.0]
    assert mgr.init_batch(np.array([5, 6, 7], dtype=np.uint32), DT, 0.0, p0, np.zeros((3, 6)), np.zeros((3, 6)),
                          type=te.MODEL_TYPES["uniform_velocity"], Q=Q, R=R, P0=np.stack([P0, P0, bad])) == 3
    b = mgr.batches()[0]
    det = _dets([[3.0, 4.0, 0.0], [103.0, 4.0, 0.0], [nan, 0.0, 0.0], [100.0, nan, 0.0], [100.0, 0.0, nan], [200.0, 0.0, 0.0],
                 [inf, 0.0, 0.0], [0.0, -inf, 0.0], [100.0, 0.0, inf]])
    for cell, wide in ((6.0, 0), (1.0, 2)):                                # the indefinite slot is neither narrow nor wide
        r = b.associate(_cuda(det, np.float64), 0.0, gate=25.0, rounds=16, cell=cell)     # d2 == gate exactly: a candidate
        torch.cuda.synchronize()
        assert list(r.det_of_slot.cpu().numpy()) == [0, 1, -1] and list(r.slot_of_det.cpu().numpy()) == [0, 1] + [-1] * 7
        assert _bits(r.d2_of_slot.cpu().numpy()).tolist() == _bits(np.array([25.0, 25.0, -1.0])).tolist()
        assert list(r.info.cpu().numpy()) == [2, 1, 1, wide]
        r = b.associate(_cuda(det, np.float64), 0.0, gate=float(np.nextafter(25.0, 0.0)), rounds=16, cell=cell)      # one ulp below: none
        torch.cuda.synchronize()
        assert list(r.det_of_slot.cpu().numpy()) == [-1, -1, -1] and list(r.info.cpu().numpy()) == [0, 1, 1, wide]
    mgr.close()


def test_every_slot_wide_and_everything_in_one_cell():
    rng = np.random.default_rng(7)
    pos_t = np.round(rng.uniform(-20, 20, (70, 3)) * 8) / 8
    pos_d = np.concatenate([pos_t[:50] + np.round(rng.normal(0, 0.5, (50, 3)) * 32) / 32, np.round(rng.uniform(-20, 20, (30, 3)) * 8) / 8])
    pos_d = pos_d[rng.permutation(80)]
    wide = _edge(pos_t, pos_d, gate=4.0, cell=2.0 ** -10)
    assert wide[-1][3] == 70
    one = _edge(np.abs(pos_t), np.abs(pos_d), gate=4.0, cell=1e6)
    assert one[-1][3] == 0
    mid = _edge(pos_t, pos_d, gate=4.0, cell=2.5)
    _same_bytes(wide, mid, "wide against narrow", skip_wide=True)


def test_planted_exact_ties_across_cells_and_buckets():
    # two detections at the same d2 of one target, in different cells (cell 2.5: coordinates -1 and 0): the lower index wins
    out = _edge([[0.0, 0, 0], [10.0, 0, 0]], [[11.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [9.0, 0, 0]], gate=4.0, cell=2.5)
    assert list(out[2][:2]) == [1, 0]
    # two targets at the same d2 of one detection, in different cells (9 / 2.5 -> 3, 11 / 2.5 -> 4): the lower slot wins
    out = _edge([[0.0, 0, 0], [11.0, 0, 0], [9.0, 0, 0]], [[10.0, 0, 0]], gate=4.0, cell=2.5)
    assert list(out[2][:3]) == [-1, 0, -1] and list(out[4]) == [1] and list(out[-1]) == [1, 1, 1, 0]
    # across two batches of a manager (19 / 2.5 -> 7, 21 / 2.5 -> 8): the lower batch wins
    for buckets in BUCKETS:
        os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)
        if buckets is not None:
            os.environ["TE_ASSOC_GRID_BUCKETS"] = str(buckets)
        try:
            mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
        finally:
            os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)
        w1 = _unit_world(np.array([[0.0, 0, 0], [19.0, 0, 0]]), name="uniform_acceleration", mgr=mgr, ids=np.array([1, 2], dtype=np.uint32))
        w2 = _unit_world(np.array([[21.0, 0, 0], [40.0, 0, 0]]), name="uniform_velocity", mgr=mgr, ids=np.array([3, 4], dtype=np.uint32))
        w1.init(); w2.init()
        assert len(mgr.batches()) == 2
        r = mgr.associate(_cuda(_dets([[41.0, 0, 0], [20.0, 0, 0]]), np.float64), 0.0, gate=4.0, rounds=16, cell=2.5)
        torch.cuda.synchronize()
        assert list(r.batch_of_det.cpu().numpy()) == [1, 0] and list(r.slot_of_det.cpu().numpy()) == [1, 1]
        assert list(r.det_of_slot[0].cpu().numpy()[:2]) == [-1, 1] and list(r.det_of_slot[1].cpu().numpy()[:2]) == [-1, 0]
        assert _bits(r.d2_of_det.cpu().numpy()).tolist() == _bits(np.array([1.0, 1.0])).tolist()
        assert list(r.info.cpu().numpy()) == [2, 1, 1, 0]
        mgr.close()


@pytest.mark.parametrize("cell", [16.0, 3.0])
def test_chain_scene_rounds(cell):
    """one match per round, settled at round L; cell 16: every slot narrow, cell 3: every slot wide"""
    L = 6
    t, d = ar.chain(L)
    pos_t, pos_d = np.stack([t, np.zeros(L), np.zeros(L)], axis=1), np.stack([d, np.zeros(L), np.zeros(L)], axis=1)
    for rounds in range(1, L + 2):
        out = _edge(pos_t, pos_d, gate=200.0, cell=cell, rounds=rounds)
        assert list(out[-1]) == [min(rounds, L), min(rounds, L), int(rounds >= L), 0 if cell == 16.0 else L]


# ---------------------------------------------------------------------------------------------------------------- 4. beyond the old cap
def test_a_frame_beyond_the_brute_force_cap():
    n, M = 130, 66000
    assert M > ar.MAX_DETECTIONS
    w = _scaled_world("uniform_velocity", "f64", "301", n, seed=4)
    tl, ts = _twin_tables(w)
    rng = np.random.default_rng(4)
    det = _dets(np.round(rng.uniform(-0.5, 8.5, (M, 3)) * 1024) / 1024)
    near = _planted(w, tl, 300, 4)
    det[rng.permutation(M)[:300]] = near
    b = _init(w)
    r = b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=16, cell=CELL)
    info = _check_twin(w, r, det, ts, GATE, 16, CELL, "66000 detections")
    assert info[0] > 100 and info[3] == len(range(0, n, 7))
    with pytest.raises(RuntimeError, match="M must be 0..65536"):
        b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=16)
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- 5. two identical calls
def test_two_identical_calls_give_the_same_bytes():
    w = _scaled_world("angular_rates", "f64", "301", 300, seed=9)
    tl, ts = _twin_tables(w)
    det = _cuda(_planted(w, tl, 300, 9), np.float64)
    b = _init(w, 4)
    first = _arrays(b.associate(det, DT, gate=GATE, rounds=3, cell=CELL))
    for _ in range(2):
        _same_bytes(first, _arrays(b.associate(det, DT, gate=GATE, rounds=3, cell=CELL)), "repeat")
    # the host form: the device form's pairing, ids translated, unmatched ascending
    rh = b.associate(det.cpu().numpy(), DT, gate=GATE, rounds=3, cell=CELL)
    sod = first[4]
    assert np.array_equal(rh.slot_of_det, sod) and np.array_equal(_bits(rh.d2_of_det), _bits(first[5])) and list(rh.info) == list(first[6])
    assert rh.matched == int((sod >= 0).sum()) and np.array_equal(rh.unmatched, np.nonzero(sod < 0)[0])
    assert np.array_equal(rh.ids_of_det[sod >= 0], w.ids[sod[sod >= 0]]) and (rh.ids_of_det[sod < 0] == 0xffffffff).all()
    rm = w.mgr.associate(det.cpu().numpy(), DT, gate=GATE, rounds=3, cell=CELL)
    assert np.array_equal(rm.slot_of_det, sod) and np.array_equal(rm.ids_of_det, rh.ids_of_det) and (rm.batch_of_det[sod >= 0] == 0).all()
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- 6. into the tick
TICK_GATE, TICK_CELL = 50.0, 1.25       # reach = sqrt(50 S_aa) is about 1 m at these S


@pytest.mark.parametrize("name,dtype,layout", [("uniform_acceleration", "f64", "301shared"), ("angular_rates", "f32", "301"),
                                                ("angular_velocities", "f64", "packed")])
def test_associate_then_step_equals_the_labelled_step(name, dtype, layout):
    n = 130
    w, tw = World(name, dtype, layout, n, seed=2), World(name, dtype, layout, n, seed=2)
    b, tb = w.init(), tw.init()
    rng = np.random.default_rng(8)
    tdt = b.torch_dtype()
    for s in range(3):
        meas = _labelled(w, rng, s)
        perm = rng.permutation(n)
        r = b.associate(_cuda(meas[perm], np.float64), DT, gate=TICK_GATE, rounds=16, cell=TICK_CELL)
        b.step(DT, r.meas, r.has_meas)
        tb.step(DT, _cuda(meas.T, np.float64).to(tdt).contiguous(), torch.ones(n, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        assert np.array_equal(r.slot_of_det.cpu().numpy(), perm) and list(r.info.cpu().numpy())[0] == n
    x, P = w.mgr.get_state_batch(w.ids)
    tx, tP = tw.mgr.get_state_batch(tw.ids)
    assert np.array_equal(_bits(x), _bits(tx)) and np.array_equal(_bits(P), _bits(tP))
    w.mgr.close(); tw.mgr.close()


def test_mixed_manager_through_step_sequence_all_and_several_shards_refuse():
    def build():
        mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        ws = [World("angular_rates", "f64", "301", 70, seed=3, mgr=mgr, ids=np.arange(70, dtype=np.uint32)),
              World("angular_velocities", "f64", "301", 65, seed=4, mgr=mgr, ids=np.arange(65, dtype=np.uint32) + 1000)]
        ws[1].p0[:, 2] += 4.0
        for w in ws:
            w.init()
        return mgr, ws
    mgr, ws = build()
    tmgr, tws = build()
    rng = np.random.default_rng(9)
    order = [te.MODEL_TYPES[w.name] for w in ws]
    ws_by_batch = [ws[order.index(b.type)] for b in mgr.batches()]
    for s in range(2):
        per = [_labelled(w, rng, s) for w in ws_by_batch]
        frame = np.concatenate(per)
        perm = rng.permutation(len(frame))
        r = mgr.associate(_cuda(frame[perm], np.float64), DT, gate=TICK_GATE, rounds=16, cell=TICK_CELL)
        mgr.step_sequence_all(DT, r.meas, r.has_meas, n_ticks=1)
        tmgr.step_sequence_all(DT, [_cuda(m.T[None], np.float64) for m in per],
                               [torch.ones((1, m.shape[0]), dtype=torch.uint8, device="cuda") for m in per], n_ticks=1)
        torch.cuda.synchronize()
        assert list(r.info.cpu().numpy())[0] == len(frame) and list(r.info.cpu().numpy())[2] == 1
    for w, t in zip(ws, tws):
        x, P = mgr.get_state_batch(w.ids)
        tx, tP = tmgr.get_state_batch(t.ids)
        assert np.array_equal(_bits(x), _bits(tx)) and np.array_equal(_bits(P), _bits(tP))
    mgr.close(); tmgr.close()
    sh = te.TargetManager(dtype="f64", devices=[0, 0])
    with pytest.raises(RuntimeError, match="shards"):
        sh.associate(_cuda(_dets([[0.0, 0, 0]]), np.float64), DT, gate=TICK_GATE, rounds=4, cell=TICK_CELL)
    with pytest.raises(RuntimeError, match="shards"):
        sh.associate(_dets([[0.0, 0, 0]]), DT, gate=TICK_GATE, rounds=4, cell=TICK_CELL)
    sh.close()


def test_captured_graph_of_associate_and_step_replays():
    """associate(cell) -> step captured in the caller's graph -- a linear chain of kernel launches -- after a warm call of the same
    size: two replays leave the batch bit for bit where two eager rounds leave a twin"""
    name, n = "uniform_acceleration", 130
    stream = torch.cuda.Stream()
    ws = []
    with torch.cuda.stream(stream):
        for _ in range(2):
            w = World(name, "f64", "301", n, seed=5)
            w.init()
            ws.append(w)
        rng = np.random.default_rng(10)
        frames = [_labelled(ws[0], rng, s)[rng.permutation(n)] for s in range(3)]
        det = [_cuda(f, np.float64) for f in frames]
        buf = det[0].clone()
        outs = []
        for w in ws:
            r = w.b.associate(buf, DT, gate=TICK_GATE, rounds=4, cell=TICK_CELL)
            w.b.step(DT, r.meas, r.has_meas)
            outs.append(r)
        stream.synchronize()
        eager, graphed = ws
        for s in (1, 2):
            buf.copy_(det[s])
            r = eager.b.associate(buf, DT, gate=TICK_GATE, rounds=4, out=outs[0], cell=TICK_CELL)
            eager.b.step(DT, r.meas, r.has_meas)
        stream.synchronize()
        want = eager.mgr.get_state_batch(eager.ids)
        g = torch.cuda.CUDAGraph()
        buf.copy_(det[1])
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            r = graphed.b.associate(buf, DT, gate=TICK_GATE, rounds=4, out=outs[1], cell=TICK_CELL)
            graphed.b.step(DT, r.meas, r.has_meas)
        g.replay()
        buf.copy_(det[2])
        g.replay()
        stream.synchronize()
        got = graphed.mgr.get_state_batch(graphed.ids)
        assert list(outs[1].info.cpu().numpy())[0] == n
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    for w in ws:
        w.mgr.close()
