"""Duplicate tracks on the device (target_manager_find_duplicates_dev, target_manager_retire_duplicates) on COUPLED
tracks: dense covariances with every word between two axes populated, a coupled Q, a non-zero acceleration state, and an ordinary
dt -- what test_gpu_track_merge's fresh diagonal worlds never give the table kernel's Sigma words or the pair's inverse.

a. FRESH COUPLED WORLDS, BIT FOR BIT THE TWIN (tests/track_merge_ref.py).  The scenes of tests/track_merge_coupled_scenes.py in
   the dense layouts, per-target P0 rounded to the batch's precision on the CPU, dt = 2^-6: every product of the table is exact,
   so the twin forms the device's doubles; every output array and info by bits; planned buckets, 1 and 4 give the same bytes.
   Before the device is touched the twin shows that the scene is not vacuous (matched pairs, correlated pair sums, a pair that
   the gate alone rejects, a wide row, a row with too few hits).
b. FILTERED TRACKS AT dt = 0.01 AGAINST THE EXTENDED-PRECISION REFERENCE (tests/track_merge_highprec_ref.py).  Six ticks; a twin
   is fed its partner's measurement plus millimetre noise, displaced by a constant planted offset (centimetres: what spreads the
   pairs' d2 over the gate -- with the noise alone every twin's d2 would lie below 0.01 and no two could be told apart in float32).
   x and P are read back; every returned d2 is held to the reference within the ALLOWANCE -- 8 x the largest deviation of the
   same-precision twin from the reference over the pairs with d2 <= 4 gate of the same inputs, |d2 - ref| / max(ref, 1), floor
   2^-50, printed -- and partners, dup and info are exactly those of sorted greedy on the reference's costs.  Before the call the
   state read back must be separated: every d2 up to 4 gate from every other and from the gate, every box comparison of those
   pairs and every narrow / wide comparison from its limit, by more than 100 x the allowance.  (A pair beyond 4 gate is no
   candidate whatever its box says.)  Figures of an MI355X run: profiles/track_merge_tolerances.txt.
c. CROSS-MODEL PAIRS: uniform velocity and uniform acceleration in one manager at 3 lanes, 70 and 65 targets, twins planted across
   the two batches; bit for bit the twin.
d. RETIRE on a coupled world against the twin's list and a second manager cleaned with erase_batch, by snapshot."""
import numpy as np
import pytest

import associate_ref as ar
import track_merge_coupled_scenes as cs
import track_merge_highprec_ref as hp
import track_merge_ref as tm
from test_gpu_associate import DENSE, DT, World, _bits, _cuda, _np_t
from test_gpu_associate_grid import _init
from test_gpu_track_merge import BUCKETS, _arrays, _check, _raise_counters, _same_bytes, _snapshot, _want, lr_erase

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

GATE = cs.GATE
MIN_HITS = cs.MIN_HITS
MODELS = list(DENSE)


# ---------------------------------------------------------------------------------------------------------------- a. bit for bit
def _coupled_world(name, dtype, layout, n, seed, mgr=None, ids=None, origin=(0.0, 0.0, 0.0)):
    w = World(name, dtype, layout, n, seed, mgr=mgr, ids=ids)
    w.scene = cs.scene(name, dtype, n, seed, DT, origin=origin)
    return cs.fill_world(w, w.scene)


def _rows_of(w, dt=DT):
    """the twin's rows from the state a fresh world holds, the class matrices as the device holds them"""
    T = _np_t(w.dtype)
    s = w.scene
    R = w.R.astype(T).astype(np.float64)
    return tm.rows(s.x, s.P0, s.Q, R, dt, w.name, T)


def _not_vacuous(rows, hits, miss, cell, n, what):
    """on the twin, before the device is touched"""
    want, partner, D = _want(rows, hits, miss, GATE, cell, 16, MIN_HITS, [n])
    cls = tm.classes(rows[0], rows[1], rows[2], hits, MIN_HITS, GATE, cell)
    d2, inbox, ok = tm.pair_terms(rows[0], rows[1], GATE)
    e = cls == tm.ELIGIBLE
    lo = np.nonzero((partner >= 0) & (partner > np.arange(len(partner))))[0]
    assert 8 * len(lo) >= n, (what, len(lo))
    C = rows[1][lo] + rows[1][partner[lo]]
    assert 3 * int((cs.correlation(C) >= 0.3).sum()) >= len(lo), what
    with np.errstate(invalid="ignore"):
        assert (ok & e[:, None] & e[None, :] & inbox & (d2 > GATE)).any(), what           # rejected by the gate alone
    assert (cls == tm.WIDE).any() and (rows[2] & (hits < MIN_HITS)).any(), what
    return want


def _check_state(w, what):
    """the device holds the scene's words on the chains the table reads"""
    N, K = ar.MODEL_NK[w.name]
    T = _np_t(w.dtype)
    gx, gP = w.mgr.get_state_batch(w.ids)
    ch = np.array([r + i * K for i in range(N // K) for r in range(3)])
    assert np.array_equal(gx[:, ch], w.scene.x.astype(T)[:, ch]), what
    assert np.array_equal(gP[:, ch][:, :, ch], w.scene.P0.astype(T)[:, ch][:, :, ch]), what


def _run_coupled(name, dtype, layout, n, seed, buckets_list=(None,)):
    cell = cs.CELL[dtype]
    hits, miss = cs.counters(n)
    res = []
    for buckets in buckets_list:
        what = "%s %s %s n %d buckets %s" % (name, dtype, layout, n, buckets)
        w = _coupled_world(name, dtype, layout, n, seed)
        rows = _rows_of(w)
        want = _not_vacuous(rows, hits, miss, cell, n, what)
        _init(w, buckets)
        _check_state(w, what)
        _raise_counters(w.mgr, [(hits, miss)])
        for rounds in (1, 16):
            got = _arrays(w.mgr.find_duplicates(DT, GATE, cell, rounds=rounds, min_hits=MIN_HITS), [n])
            _check(got, want if rounds == 16 else _want(rows, hits, miss, GATE, cell, rounds, MIN_HITS, [n])[0], what + " rounds %d" % rounds)
            res.append(got)
        w.mgr.close()
    for k in range(2, len(res)):
        _same_bytes(res[k % 2], res[k], (name, n, k))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["full", "packed"])
@pytest.mark.parametrize("name", MODELS)
def test_fresh_coupled_worlds_are_the_twin_bit_for_bit(name, layout, dtype):
    _run_coupled(name, dtype, layout, 65 if layout == "packed" else 130, seed=MODELS.index(name))


@pytest.mark.parametrize("name,dtype,layout", [("uniform_acceleration", "f64", "packed"), ("angular_velocities", "f32", "full")])
def test_coupled_world_under_planned_one_and_four_buckets(name, dtype, layout):
    _run_coupled(name, dtype, layout, 130, seed=5, buckets_list=BUCKETS)


# ---------------------------------------------------------------------------------------------------------------- b. filtered tracks
TICKS = 6
CELL_B = 0.5
FILTERED = [(name, dtype, layout) for name in ("uniform_velocity", "uniform_acceleration") for dtype in ("f64", "f32")
            for layout in ("full", "packed")] + [("uniform_acceleration", "f64", "301"), ("uniform_acceleration", "f64", "301shared")]


def _kf_covariance(name, P0, Q, R, ticks):
    """the covariance recursion of the linear models (data-independent), only to SIZE the planted offsets: [N, N] after `ticks`
    measured ticks of DT"""
    N, K = ar.MODEL_NK[name]
    A = hp.transition(DT, name).astype(np.float64)
    H = np.eye(K, N)
    P = np.array(P0, dtype=np.float64)
    for _ in range(ticks):
        P = A @ P @ A.T + Q
        G = P @ H.T @ np.linalg.inv(H @ P @ H.T + R)
        P = (np.eye(N) - G @ H) @ P
    return P


def filtered_scene(name, dtype, layout, n, seed):
    """the World, the measurement stream [TICKS, n, 7] and the measured mask [n]: rows 4f + 1 (float32: 8f + 1) are twins of the row before (the same P0,
    velocity and acceleration; displaced by the planted offset, which their measurements keep), rows 16g + 10 are never measured
    and start from 16 x the covariance (wide at CELL_B); the dense layouts get a coupled P0 per family"""
    w = World(name, dtype, layout, n, seed)
    T = _np_t(dtype)
    rng = np.random.default_rng(500 + seed)
    N, K = ar.MODEL_NK[name]
    i = np.arange(n)
    pos = np.stack([i % 8, (i // 8) % 8, i // 64], axis=1) + rng.uniform(-0.2, 0.2, (n, 3))
    w.p0[:, :3] = pos
    if N // K == 3:
        w.a0[:, :3] = rng.uniform(-3, 3, (n, 3))
    dense = layout in ("full", "packed")
    lost = (i % 16 == 10) if layout != "301shared" else np.zeros(n, dtype=bool)
    w.p0[lost, 2] += 20.0 + 5.0 * (i[lost] // 16)                # (far from everything: their broad Sigma would fill the window)
    ratios = cs.RATIOS["f32"] if dtype == "f32" else (1.0, 3.0, 12.0)
    if dense:
        P0 = np.zeros((n, N, N))
        for k in range(n):
            if k % 4 == 1:
                G = np.eye(N) + 1e-3 * rng.normal(size=(N, N))
                P0[k] = G @ P0[k - 1] @ G.T
            else:
                P0[k] = cs.coupled_p(rng, name, ratios[(k // 4) % len(ratios)], rest=1e-2) * (16.0 if lost[k] else 1.0)
            P0[k] = 0.5 * (P0[k] + P0[k].T)
        w.P0 = P0.astype(T).astype(np.float64)
    elif lost.any():
        P0 = np.broadcast_to(w.P0, (n, N, N)).copy()
        P0[lost] *= 16.0
        w.P0 = P0
    P0n = np.broadcast_to(w.P0, (n, N, N))
    twins = np.arange(1, n, 4 if dtype == "f64" else 8)          # float32: fewer pairs, wider apart -- its allowance is 10^7 x the other
    vals = 0.05 + (np.arange(len(twins)) + 0.5) * (0.85 * GATE / len(twins))
    vals[3::10] = GATE * (1.1 + 2.4 * rng.uniform(size=len(vals[3::10])))
    vals = rng.permutation(vals)
    off = np.zeros((n, 3))
    for v, k in zip(vals, twins):
        P = _kf_covariance(name, P0n[k - 1], w.Q, w.R, TICKS)
        _, Sg, _ = hp.rows(np.zeros((1, N)), P[None], w.Q, 0.01, name)
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        off[k] = np.linalg.cholesky(2.0 * Sg[0].astype(np.float64)) @ u * np.sqrt(v)
        w.p0[k, :3] = w.p0[k - 1, :3] + off[k]
        w.v0[k], w.a0[k] = w.v0[k - 1], w.a0[k - 1]
    meas = np.zeros((TICKS, n, 7)); meas[:, :, 6] = 1.0
    for s in range(TICKS):
        t = DT * (s + 1)
        m = w.p0[:, :3] + w.v0[:, :3] * t + 0.5 * w.a0[:, :3] * t * t * (N // K == 3) + rng.normal(0, 0.02, (n, 3))
        m[twins] = m[twins - 1] + off[twins] + rng.normal(0, 0.0005, (len(twins), 3))
        meas[s, :, :3] = m
    return w, meas, ~lost


def reference_of(w, x, P, hits, cell, dt=0.01):
    """from the state read back: the allowance, the margins, and what sorted greedy on the reference's costs gives"""
    T = _np_t(w.dtype)
    Q, R = w.Q.astype(T).astype(np.float64), w.R.astype(T).astype(np.float64)
    zr, Sr, vr = hp.rows(x, P, Q, dt, w.name, R=R)
    C, nu, d2r = hp.pairs(zr, Sr)
    zt, St, vt = tm.rows(x, P, Q, R, dt, w.name, T)
    assert np.array_equal(vr, vt)
    d2t, _, _ = tm.pair_terms(zt, St, GATE)
    v2 = vr[:, None] & vr[None, :]
    dev = hp.deviation(np.where(v2, d2t, np.nan), np.where(v2, d2r, np.nan), 4 * GATE)
    tol = hp.allowance(dev)
    margins = hp.separation(zr, Sr, vr, GATE, cell)
    Dr, cls = hp.decide(zr, Sr, vr, hits, 0, GATE, cell)
    return tol, margins, Dr, cls, d2r


def _step_filtered(w, b, meas, measured):
    tdt = b.torch_dtype()
    if w.layout == "301shared":
        b.step_sequence(DT, _cuda(meas.transpose(0, 2, 1), np.float64), use_graph=True)
        assert b.shared_axes == 1 and b.uniform_tiles > 0
        return
    mask = _cuda(measured.astype(np.uint8), np.uint8)
    for s in range(TICKS):
        b.step(DT, _cuda(meas[s].T, np.float64).to(tdt).contiguous(), mask)


@pytest.mark.parametrize("name,dtype,layout", FILTERED)
def test_filtered_tracks_at_an_ordinary_dt_against_the_reference(name, dtype, layout):
    n = 65 if dtype == "f32" or layout == "packed" else 130
    w, meas, measured = filtered_scene(name, dtype, layout, n, seed=1)
    b = _init(w)
    _step_filtered(w, b, meas, measured)
    x, P = w.mgr.get_state_batch(w.ids)
    miss, hits = b.track_counts()
    what = "%s %s %s n %d" % (name, dtype, layout, n)
    tol, margins, Dr, cls, d2r = reference_of(w, x, P, hits, CELL_B)
    print("%s: allowance %.3e; margins: d2 %.3e, box %.3e, class %.3e" % (what, tol, margins[0], margins[1], margins[2]))
    assert min(margins) > 100 * tol, (what, margins, tol)                     # separated: before the call under test
    partner = hp.greedy(Dr)
    p2, info = tm.match(Dr, 16)
    assert np.array_equal(p2, partner) and info[2] == 1
    pairs = int((partner >= 0).sum()) // 2
    wide = int((cls == hp.WIDE).sum())
    with np.errstate(invalid="ignore"):
        beyond = int((np.triu(np.ones((n, n), dtype=bool), 1) & (d2r > GATE) & (d2r <= 4 * GATE)).sum())
    assert pairs >= n // 16 and beyond >= 1 and (wide >= 1 or layout == "301shared"), (what, pairs, beyond, wide)
    got = _arrays(w.mgr.find_duplicates(0.01, GATE, CELL_B, rounds=16, min_hits=0), [n])
    assert list(got[4]) == [pairs, info[1], 1, wide], (what, got[4], info, wide)
    assert np.array_equal(got[1], np.where(partner >= 0, 0, -1)) and np.array_equal(got[2], partner), what
    assert np.array_equal(got[0], tm.weaker(partner, hits, miss)), what
    m = partner >= 0
    assert (got[3][~m] == -1.0).all(), what
    ref = d2r[np.nonzero(m)[0], partner[m]]
    err = float((np.abs(got[3][m].astype(np.longdouble) - ref) / np.maximum(ref, 1)).max())
    print("%s: d2 error %.3e (allowed %.3e, share %.3f) over %d matched rows" % (what, err, tol, err / tol, int(m.sum())))
    assert err <= tol, what
    if layout == "301shared":
        assert b.shared_axes == 1 and b.uniform_tiles > 0
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- c. cross-model pairs
def _cross_worlds(buckets=None):
    """uniform velocity (70) and uniform acceleration (65) in one manager at 3 lanes; rows 8g + 7 of the second model are tracks of
    the objects that rows 8g + 7 of the first model follow: the same velocity, a planted offset between the predicted positions"""
    import os
    os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)
    if buckets is not None:
        os.environ["TE_ASSOC_GRID_BUCKETS"] = str(buckets)
    try:
        mgr = te.TargetManager(dtype="f64", lanes_per_target=3)
    finally:
        os.environ.pop("TE_ASSOC_GRID_BUCKETS", None)
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    ws = _cross_scenes(mgr)
    for w in ws:
        w.init()
    by_type = {te.MODEL_TYPES[w.name]: w for w in ws}
    return mgr, [by_type[b.type] for b in mgr.batches()]


def _cross_scenes(mgr=None):
    w1 = _coupled_world("uniform_velocity", "f64", "full", 70, 11, mgr=mgr, ids=np.arange(70, dtype=np.uint32) + 100)
    w2 = _coupled_world("uniform_acceleration", "f64", "full", 65, 12, mgr=mgr, ids=np.arange(65, dtype=np.uint32) + 1000, origin=(0.0, 0.0, 2.0))
    s1, s2 = w1.scene, w2.scene
    rng = np.random.default_rng(13)
    z1, S1, _ = hp.rows(s1.x, s1.P0, s1.Q, DT, s1.name)
    _, S2, _ = hp.rows(s2.x, s2.P0, s2.Q, DT, s2.name)
    rows_x = np.arange(7, 65, 8)
    vals = rng.permutation(0.05 + (np.arange(len(rows_x)) + 0.5) * (0.85 * GATE / len(rows_x)))
    for v, k in zip(vals, rows_x):
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        o = np.linalg.cholesky((S1[k] + S2[k]).astype(np.float64)) @ u * np.sqrt(v)
        s2.vel[k] = s1.vel[k]
        z = z1[k].astype(np.float64) + o - s2.vel[k] * DT - 0.5 * s2.acc[k] * DT * DT
        s2.pos[k] = np.round(z * 2.0 ** 30) / 2.0 ** 30
    s2.x = cs.state(s2.name, s2.pos, s2.vel, s2.acc)
    cs.fill_world(w2, s2)
    return [w1, w2]


def test_cross_model_pairs_in_a_dense_layout():
    res = []
    for buckets in (None, 4):
        mgr, ws = _cross_worlds(buckets)
        sizes = [w.n for w in ws]
        per = [cs.counters(w.n) for w in ws]
        hits, miss = np.concatenate([h for h, m in per]), np.concatenate([m for h, m in per])
        parts = [_rows_of(w) for w in ws]
        rows = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
        cell = cs.CELL["f64"]
        want, partner, D = _want(rows, hits, miss, GATE, cell, 16, MIN_HITS, sizes)
        batch_of = np.repeat(np.arange(2), sizes)
        m = partner >= 0
        cross = int((batch_of[m] != batch_of[partner[m]]).sum()) // 2
        assert cross >= 4 and want[4][0] > cross + 8 and want[4][3] > 0, (cross, want[4])
        for w in ws:
            _check_state(w, "cross " + w.name)
        _raise_counters(mgr, per)
        got = _arrays(mgr.find_duplicates(DT, GATE, cell, rounds=16, min_hits=MIN_HITS), sizes)
        _check(got, want, "cross buckets %s" % buckets)
        res.append(got)
        mgr.close()
    _same_bytes(res[0], res[1], "cross buckets")


# ---------------------------------------------------------------------------------------------------------------- d. retire
def test_retire_duplicates_on_a_coupled_world():
    name, dtype, layout, n = "uniform_acceleration", "f64", "packed", 130
    hits, miss = cs.counters(n)
    cell = cs.CELL[dtype]
    wa, wb = _coupled_world(name, dtype, layout, n, 5), _coupled_world(name, dtype, layout, n, 5)
    _init(wa); _init(wb)
    for w in (wa, wb):
        _raise_counters(w.mgr, [(hits, miss)])
    A, B = wa.mgr, wb.mgr
    rows = _rows_of(wa)
    dup, partner, d2, info, D = tm.find(rows[0], rows[1], rows[2], hits, miss, GATE, cell, 16, MIN_HITS)
    retired, kept, after = tm.retire(dup, partner, [n], [wa.ids])
    assert len(retired) == info[0] >= n // 8 and info[3] > 0
    assert (np.nonzero(dup)[0] < n - len(retired)).any()                                     # a survivor is moved into a hole
    assert _snapshot(A) == _snapshot(B)
    out = A.retire_duplicates(DT, GATE, cell, rounds=16, min_hits=MIN_HITS)
    assert B.erase_batch(retired) == len(retired)
    assert np.array_equal(out.retired_ids, retired) and np.array_equal(out.kept_ids, kept)
    assert [out.retired, out.rounds_run, out.settled, out.wide] == [info[0], info[1], info[2], info[3]]
    assert np.array_equal(A.batches()[0].slot_ids(), after[0])
    assert _snapshot(A) == _snapshot(B)
    got_m, got_h = A.batches()[0].track_counts()
    assert np.array_equal(got_h, lr_erase(hits, dup)) and np.array_equal(got_m, lr_erase(miss, dup))
    A.close(); B.close()
