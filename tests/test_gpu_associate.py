"""Association of unlabelled detections on the device (target_batch_associate[_dev], target_manager_associate[_dev])
against the NumPy twin tests/associate_ref.py.

d2: every d2 the call exposes (d2_of_slot and d2_of_det of every matched pair, under an infinite gate, on filters that have been
stepped) against the longdouble twin fed with get_state's x and P and the class matrices as the device holds them.  TOLERANCE, not
fixed here: 8 x the largest deviation of the same-precision twin from the longdouble twin over ALL pairs of the same inputs, as
|d2 - ref| / max(ref, 1); measured per (model, precision), printed by the test and kept in profiles/associate_tolerances.txt.
Measured on an MI355X run (stepped filters, dt = 0.01): f64 6.9e-14 .. 1.7e-13 (uniform_velocity / angular_velocities 6.9e-14 ..
8.2e-14, uniform_acceleration / angular_rates 1.0e-13 .. 1.7e-13); f32 3.6e-05 .. 4.8e-05 for all four models (zhat rounded to
f32 against offsets of a few sigma = 5 cm).  The device's own error was at most 0.125 of the allowance over the 301 figures that run printed.
ASSIGNMENT: exactly the twin's.  The scenes are known on the CPU (fresh targets: x = p0, v0; P = P0; positions, velocities and dt
on a binary grid, so that zhat = x + v dt is exact in f32 too): before the GPU is touched the twin asserts that all d2 up to
4 x gate differ pairwise by more than 100 x the tolerance (relative to max(d2, 1)) and that none lies that close to the gate.
Then: exact ties, rounds on the chain scene, NaN detections and an S that is not positive definite, d2 == gate built exactly, the
two d2 arrays bit-equal, chunk counts 1 and 3 identical, and the scattered output stepping a batch / a mixed manager bit for bit as
the labelled input steps a twin -- also from a captured graph."""
import os

import numpy as np
import pytest

import associate_ref as ar
from conftest import HARNESS_ORDER

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

INF = float("inf")
GATE = 9.0
DT = 2.0 ** -6                   # with positions on the 2^-10 grid and velocities on the 2^-4 grid, x + v dt is exact in f32
SIGMA = 0.05
DENSE = {"uniform_velocity": (3, 103), "uniform_acceleration": (3, 103), "angular_rates": (6, 106), "angular_velocities": (6, 106)}
LAYOUTS = ["301", "301shared", "201", "full", "packed", "classes"]
CASES = [(m, d, l) for m in HARNESS_ORDER for d in ("f64", "f32") for l in LAYOUTS if not (l == "301shared" and d == "f32")]
TOL_FLOOR = {"f64": 2.0 ** -50, "f32": 2.0 ** -50}     # never below a few ulps of the double d2 itself


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np_t(dtype):
    return np.float32 if dtype == "f32" else np.float64


def _matrices(name, layout):
    """Q, R, P0 of the tests: sigma = 5 cm per position axis; anisotropic where the layout allows it, the position axes coupled in R
    where it stores the words between them; two classes for "classes" (the second with 4 R).  cond(S) stays below 10^3."""
    N, K = ar.MODEL_NK[name]
    Q = 1e-6 * np.eye(N)
    P0 = 1e-2 * np.eye(N)
    r = np.full(K, SIGMA ** 2)
    if layout != "301shared":
        r[:3] = [2.5e-3, 4e-3, 1e-2]
    R = np.diag(r)
    if layout in ("full", "packed"):
        R[0, 1] = R[1, 0] = 1e-3
        R[1, 2] = R[2, 1] = -5e-4
    if layout == "classes":
        return np.stack([Q, Q]), np.stack([R, 4 * R]), np.stack([P0, P0])
    return Q, R, P0


def _grid(a, step):
    return np.round(np.asarray(a) / step) * step


class World:
    """n fresh targets of one model on a jittered lattice (spacing 1 m; a few pairs 0.125 m apart: contested ground), moving"""

    def __init__(self, name, dtype, layout, n, seed, chunks=None, ids=None, mgr=None):
        self.name, self.dtype, self.layout, self.n = name, dtype, layout, n
        rng = np.random.default_rng(seed)
        i = np.arange(n)
        pos = np.stack([i % 8, (i // 8) % 8, i // 64], axis=1).astype(np.float64) + rng.uniform(-0.2, 0.2, (n, 3))
        close = (i % 16 == 5) & (i > 0)
        pos[close] = pos[np.maximum(i - 1, 0)][close] + [0.125, 0.0, 0.0]
        self.p0 = np.zeros((n, 7)); self.p0[:, :3] = _grid(pos, 2.0 ** -10); self.p0[:, 6] = 1.0
        self.v0 = np.zeros((n, 6)); self.v0[:, :3] = _grid(rng.uniform(-2, 2, (n, 3)), 2.0 ** -4)
        self.a0 = np.zeros((n, 6))
        self.Q, self.R, self.P0 = _matrices(name, layout)
        self.cls = (i % 2).astype(np.uint32) if layout == "classes" else None
        self.ids = (np.arange(n, dtype=np.uint32) * 3 + 11) if ids is None else ids
        self.mgr, self.chunks = mgr, chunks

    def init(self):
        """the manager (TE_ASSOC_COL_CHUNKS is read when it is created) and the targets; returns the batch"""
        name, layout = self.name, self.layout
        if self.mgr is None:
            if self.chunks is not None:
                os.environ["TE_ASSOC_COL_CHUNKS"] = str(self.chunks)
            try:
                lanes = {"301": 301, "301shared": 301, "201": 201, "full": DENSE[name][0], "packed": DENSE[name][1], "classes": 301}[layout]
                self.mgr = te.TargetManager(dtype=self.dtype, lanes_per_target=lanes, shared_axes=(layout == "301shared"))
            finally:
                os.environ.pop("TE_ASSOC_COL_CHUNKS", None)
            self.mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        typ = te.MODEL_TYPES[self.name]
        if self.n == 0:
            return None
        if self.cls is not None:
            assert self.mgr.init_batch_classes(self.ids, DT, 0.0, self.p0, typ, self.Q, self.R, self.P0, self.cls, self.v0, self.a0) == self.n
        else:
            assert self.mgr.init_batch(self.ids, DT, 0.0, self.p0, self.v0, self.a0, type=typ, Q=self.Q, R=self.R, P0=self.P0) == self.n
        self.b = self.mgr.batch_of_type(typ)
        return self.b

    def cpu_state(self):
        """x, P of the fresh targets as the device holds them: known without the device"""
        N, K = ar.MODEL_NK[self.name]
        x = np.zeros((self.n, N))
        x[:, 0:3] = self.p0[:, :3]
        x[:, K:K + 3] = self.v0[:, :3]
        P0 = self.P0[self.cls] if self.cls is not None else np.broadcast_to(self.P0, (self.n, N, N))
        return x, np.array(P0)

    def tables(self, x, P, dt):
        """the twin's rows in longdouble and in the batch precision; Q, R as the device holds them (rounded to the batch precision)"""
        T = _np_t(self.dtype)
        Q = self.Q[self.cls] if self.cls is not None else self.Q
        R = self.R[self.cls] if self.cls is not None else self.R
        Q, R = Q.astype(T).astype(np.float64), R.astype(T).astype(np.float64)
        x, P = x.astype(T).astype(np.float64), P.astype(T).astype(np.float64)
        return ar.table(x, P, Q, R, dt, self.name, np.longdouble), ar.table(x, P, Q, R, dt, self.name, T)


def _tolerance(dtype, tl, ts, det):
    """8 x the largest deviation of the same-precision twin from the longdouble twin over all pairs, relative to max(ref, 1)"""
    Dl, Ds = ar.d2(tl[0], tl[2], det), ar.d2(ts[0], ts[2], det)
    ok = np.isfinite(Dl.astype(np.float64))
    if not ok.any():
        return TOL_FLOOR[dtype], Dl
    dev = float((np.abs(Ds.astype(np.longdouble) - Dl)[ok] / np.maximum(Dl[ok], 1)).max())
    return max(8.0 * dev, TOL_FLOOR[dtype]), Dl


def _planted(world, tl, M, seed):
    """M detections for the world: most are a target's predicted position plus an offset whose d2 against that target is PLANTED
    (an arithmetic progression over (0.05, 0.9 gate), a tenth of them over (1.1, 3.5) gate: rejected by the gate); a tenth of the
    targets get none; second detections contest some targets; the rest is clutter far from every target.  Shuffled."""
    rng = np.random.default_rng(seed)
    n = world.n
    zhat, W = tl[0].astype(np.float64), tl[2].astype(np.float64)
    n_true = max(min(n - n // 10, M - M // 10), min(n, M, 1))
    n_con = min(n_true // 8, M - n_true)
    K = n_true + n_con
    vals = 0.05 + (np.arange(K) + 0.5) * (0.85 * GATE / max(K, 1))
    far = rng.permutation(K)[:K // 10]
    vals[far] = GATE * (1.1 + 2.4 * (np.arange(len(far)) + 0.5) / max(len(far), 1))
    vals = rng.permutation(vals)
    owners = np.concatenate([rng.permutation(n)[:n_true], rng.permutation(n)[:n_con]]).astype(int)
    det = np.zeros((M, 7)); det[:, 6] = 1.0
    for k, i in enumerate(owners):
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        q = u @ W[i] @ u
        det[k, :3] = zhat[i] + u * np.sqrt(vals[k] / q)
    for k in range(K, M):
        while True:
            c = rng.uniform(-0.5, 8.5, 3)
            if n == 0 or np.min(np.linalg.norm(zhat - c, axis=1)) > 0.8:
                break
        det[k, :3] = c
    det[:, 3:6] = rng.normal(0, 0.1, (M, 3))          # an orientation: carried along, never used for pairing
    det[:, 3:] /= np.linalg.norm(det[:, 3:], axis=1, keepdims=True)
    return det[rng.permutation(M)]


def _assert_separated(Dl, tol, gate, what):
    """all d2 up to 4 gate differ pairwise by more than 100 tol (relative to max(d2, 1)) and none lies that close to the gate"""
    v = np.sort(Dl[np.isfinite(Dl.astype(np.float64)) & (Dl <= 4 * gate)].astype(np.float64))
    if len(v) > 1:
        gap = np.diff(v) / np.maximum(v[1:], 1.0)
        assert gap.min() > 100 * tol, (what, float(gap.min()), tol)
    if len(v) and np.isfinite(gate):
        assert (np.abs(v - gate) / max(gate, 1.0)).min() > 100 * tol, what


def _check_call(world, r, det, Dl, tol, gate, rounds, what):
    """the device's result against the twin's on the longdouble costs, and the result's own consistency"""
    n, M = world.n, det.shape[0]
    want_dr, want_rd, want_info = ar.match(Dl.astype(np.float64), gate, rounds)
    torch.cuda.synchronize()
    info = r.info.cpu().numpy()
    dos, sod = r.det_of_slot.cpu().numpy()[:n], r.slot_of_det.cpu().numpy()
    d2s, d2d = r.d2_of_slot.cpu().numpy()[:n], r.d2_of_det.cpu().numpy()
    assert list(info) == want_info, (what, info, want_info)
    assert np.array_equal(dos, want_dr) and np.array_equal(sod, want_rd), what
    got = dos >= 0
    # the two scans' d2 of a matched pair: the same bits; unmatched: -1
    assert np.array_equal(_bits(d2s[got]), _bits(d2d[dos[got]])), what
    assert (d2s[~got] == -1.0).all() and (d2d[sod < 0] == -1.0).all(), what
    if got.any():
        ref = Dl[np.nonzero(got)[0], dos[got]]
        err = np.abs(d2s[got].astype(np.longdouble) - ref) / np.maximum(ref, 1)
        print("%s: d2 error %.3e (allowed %.3e) over %d pairs" % (what, float(err.max()), tol, int(got.sum())))
        assert float(err.max()) <= tol, what
        assert (d2s[got] <= gate).all(), what
    # the scattered measurements: the detection's 7 words rounded once, or the identity pose; the mask
    T = _np_t(world.dtype)
    meas, has = r.meas.cpu().numpy()[:, :n], r.has_meas.cpu().numpy()[:n]
    want = np.tile(np.array([0, 0, 0, 0, 0, 0, 1], dtype=T)[:, None], (1, n))
    want[:, got] = det[dos[got]].T.astype(T)
    assert meas.dtype == T and np.array_equal(meas.view(np.uint8), want.view(np.uint8)), what
    assert np.array_equal(has, got.astype(np.uint8)), what
    return info


# ---------------------------------------------------------------------------------------------------------------- d2 against the twin
@pytest.mark.parametrize("name,dtype,layout", CASES)
def test_d2_against_the_longdouble_twin(name, dtype, layout):
    """stepped filters (two measured ticks, so P is no longer P0 and x is off the grid), every matched pair's d2 under an infinite
    gate; N = 1 with a far detection (a large d2), N = 5 and N = 70 (two table workgroups)"""
    worst = 0.0
    for n, far in ((1, 40.0), (5, 1.0), (70, 1.0)):
        w = World(name, dtype, layout, n, seed=100 + n)
        b = w.init()
        rng = np.random.default_rng(n)
        tdt = b.torch_dtype()
        for s in range(2):
            meas = np.zeros((n, 7)); meas[:, 6] = 1.0
            meas[:, :3] = w.p0[:, :3] + w.v0[:, :3] * DT * (s + 1) + rng.normal(0, 0.02, (n, 3))
            b.step(DT, _cuda(meas.T, np.float64).to(tdt).contiguous())
        x, P = w.mgr.get_state_batch(w.ids)
        tl, ts = w.tables(x, P, 0.01)
        S = tl[1].astype(np.float64)
        assert np.linalg.cond(S).max() < 1e3
        det = np.zeros((n, 7)); det[:, 6] = 1.0
        det[:, :3] = tl[0].astype(np.float64) + rng.normal(0, SIGMA, (n, 3)) * far
        det = det[rng.permutation(n)]
        tol, Dl = _tolerance(dtype, tl, ts, det)
        worst = max(worst, tol)
        r = b.associate(_cuda(det, np.float64), 0.01, gate=INF, rounds=16)
        info = _check_call(w, r, det, Dl, tol, INF, 16, "%s %s %s n %d" % (name, dtype, layout, n))
        assert info[0] == n and info[2] == 1
        if layout == "301shared":
            assert b.shared_axes == 1
        w.mgr.close()
    print("tolerance %s %s %s: %.3e" % (name, dtype, layout, worst))


def test_d2_on_flagged_uniform_tiles_and_nothing_is_touched():
    """A shared-axes batch after a recorded sequence holds flagged uniform tiles: the table reads their words from the tiles' blocks.
    The call leaves state, flags, storage form, recordings and rejection runs as they were."""
    name, n = "uniform_acceleration", 130
    w = World(name, "f64", "301shared", n, seed=7)
    b = w.init()
    rng = np.random.default_rng(3)
    ticks = 4
    meas = np.zeros((ticks, n, 7)); meas[:, :, 6] = 1.0
    for s in range(ticks):
        meas[s, :, :3] = w.p0[:, :3] + w.v0[:, :3] * DT * (s + 1) + rng.normal(0, 0.02, (n, 3))
    b.step_sequence(DT, _cuda(meas.transpose(0, 2, 1), np.float64), use_graph=True)
    before = (b.shared_axes, b.uniform_tiles, b.graph_recordings)
    assert before[0] == 1 and before[1] > 0 and before[2] >= 1, before
    runs = b.rejection_runs().copy()
    x, P = w.mgr.get_state_batch(w.ids)
    tl, ts = w.tables(x, P, DT)
    det = np.zeros((n, 7)); det[:, 6] = 1.0
    det[:, :3] = tl[0].astype(np.float64) + rng.normal(0, SIGMA, (n, 3))
    det = det[rng.permutation(n)]
    tol, Dl = _tolerance("f64", tl, ts, det)
    r = b.associate(_cuda(det, np.float64), DT, gate=INF, rounds=16)
    _check_call(w, r, det, Dl, tol, INF, 16, "uniform tiles")
    assert (b.shared_axes, b.uniform_tiles, b.graph_recordings) == before
    assert np.array_equal(b.rejection_runs(), runs)
    x2, P2 = w.mgr.get_state_batch(w.ids)
    assert np.array_equal(_bits(x), _bits(x2)) and np.array_equal(_bits(P), _bits(P2))
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- the assignment
SHAPES = [(1, 1), (63, 67), (64, 257), (65, 1), (130, 300), (300, 257), (300, 300), (130, 0)]
SEEDS = {("f32", 300, 300): 1, ("f32", 130, 300): 1}     # where the default 0 does not separate the f32 costs (chosen on the CPU)


@pytest.mark.parametrize("name,dtype,layout", [("uniform_acceleration", "f64", "301"), ("uniform_velocity", "f32", "301"),
                                                ("angular_rates", "f32", "packed"), ("angular_velocities", "f64", "full"),
                                                ("uniform_acceleration", "f64", "301shared"), ("angular_rates", "f64", "classes")])
def test_assignment_is_the_twins(name, dtype, layout):
    for n, M in SHAPES:
        seed = SEEDS.get((dtype, n, M), 0)
        res = {}
        for chunks in (1, 3):
            w = World(name, dtype, layout, n, seed=seed, chunks=chunks)
            x, P = w.cpu_state()
            tl, ts = w.tables(x, P, DT)
            det = _planted(w, tl, M, seed)
            tol, Dl = _tolerance(dtype, tl, ts, det)
            what = "%s %s %s n %d M %d chunks %d" % (name, dtype, layout, n, M, chunks)
            _assert_separated(Dl, tol, GATE, what)           # ... before the GPU is touched
            b = w.init()
            gx, gP = w.mgr.get_state_batch(w.ids)
            T = _np_t(dtype)
            N, K = ar.MODEL_NK[name]
            ch = np.array([r + i * K for i in range(N // K) for r in range(3)])       # the position chains: all the table reads
            assert np.array_equal(gx[:, ch], x.astype(T)[:, ch]) and np.array_equal(gP[:, ch][:, :, ch], P.astype(T)[:, ch][:, :, ch]), what
            for rounds in (1, 16):
                r = b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=rounds)
                info = _check_call(w, r, det, Dl, tol, GATE, rounds, what + " rounds %d" % rounds)
                res[(chunks, rounds)] = [t.cpu().numpy().copy() for t in (r.meas, r.has_meas, r.det_of_slot, r.d2_of_slot, r.slot_of_det,
                                                                          r.d2_of_det, r.info)]
            assert info[2] == 1, what
            gr, gd = ar.greedy(Dl.astype(np.float64), GATE)
            assert np.array_equal(res[(chunks, 16)][2][:n], gr), what          # settled: sorted greedy
            if n >= 63 and M >= 67:
                assert 0 < info[0] < min(n, M), what                           # unmatched on both sides
            w.mgr.close()
        for rounds in (1, 16):                                                 # chunk counts 1 and 3: the same bytes
            for a, c in zip(res[(1, rounds)], res[(3, rounds)]):
                assert np.array_equal(a.view(np.uint8), c.view(np.uint8)), (name, n, M, rounds)


def test_empty_sides_and_the_host_form():
    mgr = te.TargetManager(dtype="f64")
    r = mgr.associate(_cuda(np.tile([0, 0, 0, 0, 0, 0, 1.0], (67, 1)), np.float64), DT, gate=GATE, rounds=4)      # no batch at all
    torch.cuda.synchronize()
    assert list(r.info.cpu().numpy()) == [0, 0, 1, 0] and (r.slot_of_det.cpu().numpy() == -1).all() and (r.batch_of_det.cpu().numpy() == -1).all()
    mgr.close()
    w = World("uniform_velocity", "f64", "301", 65, seed=1)
    b = w.init()
    r = b.associate(torch.empty((0, 7), dtype=torch.float64, device="cuda"), DT, gate=GATE, rounds=4)
    torch.cuda.synchronize()
    assert list(r.info.cpu().numpy()) == [0, 0, 1, 0] and (r.det_of_slot.cpu().numpy() == -1).all() and not r.has_meas.cpu().numpy().any()
    assert np.array_equal(r.meas.cpu().numpy(), np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0])[:, None], (1, 65)))
    # the host form: the device form's pairing, slots translated to ids, unmatched ascending
    x, P = w.cpu_state()
    tl, ts = w.tables(x, P, DT)
    det = _planted(w, tl, 67, 1)
    rd = b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=16)
    rh = b.associate(det, DT, gate=GATE, rounds=16)
    torch.cuda.synchronize()
    sod = rd.slot_of_det.cpu().numpy()
    assert np.array_equal(rh.slot_of_det, sod) and np.array_equal(_bits(rh.d2_of_det), _bits(rd.d2_of_det.cpu().numpy()))
    assert rh.matched == int((sod >= 0).sum()) == rh.info[0] and list(rh.info) == list(rd.info.cpu().numpy())
    assert np.array_equal(rh.unmatched, np.nonzero(sod < 0)[0])
    assert np.array_equal(rh.ids_of_det[sod >= 0], w.ids[sod[sod >= 0]]) and (rh.ids_of_det[sod < 0] == 0xffffffff).all()
    assert np.array_equal(rh.meas.cpu().numpy(), rd.meas.cpu().numpy()) and np.array_equal(rh.has_meas.cpu().numpy(), rd.has_meas.cpu().numpy())
    rm = w.mgr.associate(det, DT, gate=GATE, rounds=16)
    assert np.array_equal(rm.slot_of_det, sod) and np.array_equal(rm.ids_of_det, rh.ids_of_det) and (rm.batch_of_det[sod >= 0] == 0).all()
    # refusals at a live handle: ld < size, and nothing is written
    small = torch.zeros((7, 8), dtype=torch.float64, device="cuda")
    from types import SimpleNamespace
    with pytest.raises(RuntimeError, match="ld 8 < size 65"):
        b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=4, out=SimpleNamespace(meas=small, has_meas=rd.has_meas))
    assert not small.cpu().numpy().any()
    w.mgr.close()


@pytest.mark.parametrize("through", ["batch", "manager"])
def test_host_form_with_an_empty_frame_as_the_first_association(through):
    """The FIRST association of a manager is a host-form call with no detections (a legal call: a frame in which nothing was
    seen): the scratch's blocks exist all the same, so the result comes back -- nothing matched, settled, every slot without a
    measurement -- and the next frame pairs as the device form does."""
    w = World("uniform_velocity", "f64", "301", 65, seed=2)
    b = w.init()
    who = b if through == "batch" else w.mgr
    r = who.associate(np.empty((0, 7)), DT, gate=GATE, rounds=4)
    assert r.matched == 0 and list(r.info) == [0, 0, 1, 0]
    assert r.slot_of_det.shape == (0,) and r.ids_of_det.shape == (0,) and r.d2_of_det.shape == (0,) and r.unmatched.shape == (0,)
    has = r.has_meas if through == "batch" else r.has_meas[0]
    assert not has.cpu().numpy().any()
    x, P = w.cpu_state()
    tl, ts = w.tables(x, P, DT)
    det = _planted(w, tl, 67, 1)
    rh = who.associate(det, DT, gate=GATE, rounds=16)
    rd = b.associate(_cuda(det, np.float64), DT, gate=GATE, rounds=16)
    torch.cuda.synchronize()
    sod = rd.slot_of_det.cpu().numpy()
    assert (sod >= 0).any() and np.array_equal(rh.slot_of_det, sod)
    assert np.array_equal(_bits(rh.d2_of_det), _bits(rd.d2_of_det.cpu().numpy())) and rh.matched == int((sod >= 0).sum())
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- exact ties
def _unit_world(n_pos, name="uniform_velocity", dtype="f64", mgr=None, ids=None, chunks=None):
    """targets at integer positions with S = I exactly at dt = 0: P0 = I / 2, Q = R = I / 4"""
    n = len(n_pos)
    w = World(name, dtype, "301", n, seed=0, mgr=mgr, ids=ids, chunks=chunks)
    N, K = ar.MODEL_NK[name]
    w.Q, w.R, w.P0 = 0.25 * np.eye(N), 0.25 * np.eye(K), 0.5 * np.eye(N)
    w.p0[:, :3] = n_pos
    w.v0[:] = 0.0
    return w


def _dets(pos):
    d = np.zeros((len(pos), 7)); d[:, 6] = 1.0
    d[:, :3] = pos
    return d


@pytest.mark.parametrize("chunks", [1, 3])
def test_planted_exact_ties(chunks):
    # bit-identical duplicate detections: the lower index wins
    w = _unit_world(np.array([[0.0, 0, 0], [10.0, 0, 0]]), chunks=chunks)
    b = w.init()
    r = b.associate(_cuda(_dets([[11.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [11.0, 0, 0]]), np.float64), 0.0, gate=INF, rounds=16)
    torch.cuda.synchronize()
    assert list(r.det_of_slot.cpu().numpy()) == [1, 0]
    # two identical targets (slots 2 and 3 at the same place): the lower slot wins the one detection near them
    w.mgr.close()
    w = _unit_world(np.array([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0], [20.0, 0, 0]]), chunks=chunks)
    b = w.init()
    b.step(DT)                 # identically created and identically stepped (a predict-only tick): still the same bits
    r = b.associate(_cuda(_dets([[21.0, 0, 0]]), np.float64), 0.0, gate=4.0, rounds=16)
    torch.cuda.synchronize()
    assert list(r.det_of_slot.cpu().numpy()) == [-1, -1, 0, -1] and list(r.slot_of_det.cpu().numpy()) == [2]
    assert list(r.info.cpu().numpy()) == [1, 1, 1, 0]
    w.mgr.close()
    # across two batches of a manager: the lower batch wins
    mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
    w1 = _unit_world(np.array([[0.0, 0, 0], [20.0, 0, 0]]), name="uniform_acceleration", mgr=mgr, ids=np.array([1, 2], dtype=np.uint32))
    w2 = _unit_world(np.array([[20.0, 0, 0], [40.0, 0, 0]]), name="uniform_velocity", mgr=mgr, ids=np.array([3, 4], dtype=np.uint32))
    w1.init(); w2.init()
    bs = mgr.batches()
    assert len(bs) == 2
    r = mgr.associate(_cuda(_dets([[41.0, 0, 0], [21.0, 0, 0]]), np.float64), 0.0, gate=4.0, rounds=16)
    torch.cuda.synchronize()
    assert list(r.batch_of_det.cpu().numpy()) == [1, 0] and list(r.slot_of_det.cpu().numpy()) == [1, 1]
    assert list(r.det_of_slot[0].cpu().numpy()[:2]) == [-1, 1] and list(r.det_of_slot[1].cpu().numpy()[:2]) == [-1, 0]
    assert _bits(r.d2_of_det.cpu().numpy()).tolist() == _bits(np.array([1.0, 1.0])).tolist()
    mgr.close()


def test_gate_boundary_nan_detections_and_an_indefinite_s():
    # slot 2: S with a non-positive determinant, forced through its P0 (xy = 2 against diagonal 1 after Q and R: det < 0); full layout
    mgr = te.TargetManager(dtype="f64", lanes_per_target=3)
    N = 6
    Q, R, P0 = 0.25 * np.eye(N), 0.25 * np.eye(3), 0.5 * np.eye(N)
    bad = P0.copy(); bad[0, 1] = bad[1, 0] = 2.0
    p0 = np.zeros((3, 7)); p0[:, 6] = 1.0; p0[:, 0] = [0.0, 100.0, 200.0]
    ids = np.array([5, 6, 7], dtype=np.uint32)
    assert mgr.init_batch(ids, DT, 0.0, p0, np.zeros((3, 6)), np.zeros((3, 6)), type=te.MODEL_TYPES["uniform_velocity"], Q=Q, R=R,
                          P0=np.stack([P0, P0, bad])) == 3
    b = mgr.batches()[0]
    nan = float("nan")
    det = _dets([[3.0, 4.0, 0.0], [103.0, 4.0, 0.0], [nan, 0.0, 0.0], [100.0, nan, 0.0], [100.0, 0.0, nan], [200.0, 0.0, 0.0]])
    r = b.associate(_cuda(det, np.float64), 0.0, gate=25.0, rounds=16)           # d2 == gate exactly: a candidate
    torch.cuda.synchronize()
    assert list(r.det_of_slot.cpu().numpy()) == [0, 1, -1] and list(r.slot_of_det.cpu().numpy()) == [0, 1, -1, -1, -1, -1]
    assert _bits(r.d2_of_slot.cpu().numpy()).tolist() == _bits(np.array([25.0, 25.0, -1.0])).tolist()
    r = b.associate(_cuda(det, np.float64), 0.0, gate=float(np.nextafter(25.0, 0.0)), rounds=16)      # one ulp below: none
    torch.cuda.synchronize()
    assert list(r.det_of_slot.cpu().numpy()) == [-1, -1, -1] and list(r.info.cpu().numpy()) == [0, 1, 1, 0]
    r = b.associate(_cuda(det, np.float64), 0.0, gate=INF, rounds=16)            # NaN detections and the indefinite slot: never
    torch.cuda.synchronize()
    sod = r.slot_of_det.cpu().numpy()
    assert (sod[2:5] == -1).all() and r.det_of_slot.cpu().numpy()[2] == -1 and list(r.info.cpu().numpy())[0] == 2
    mgr.close()


@pytest.mark.parametrize("chunks", [1, 3])
def test_chain_scene_rounds(chunks):
    L = 6
    t, d = ar.chain(L)
    w = _unit_world(np.stack([t, np.zeros(L), np.zeros(L)], axis=1), chunks=chunks)
    b = w.init()
    det = _dets(np.stack([d, np.zeros(L), np.zeros(L)], axis=1))
    D = (d[None, :] - t[:, None]) ** 2
    for rounds in range(1, L + 2):
        r = b.associate(_cuda(det, np.float64), 0.0, gate=INF, rounds=rounds)
        torch.cuda.synchronize()
        dr, rd, info = ar.match(D, INF, rounds)
        assert list(r.info.cpu().numpy()) == info == [min(rounds, L), min(rounds, L), int(rounds >= L), 0]
        assert np.array_equal(r.det_of_slot.cpu().numpy(), dr) and np.array_equal(r.slot_of_det.cpu().numpy(), rd)
        assert np.array_equal(_bits(r.d2_of_det.cpu().numpy()[rd >= 0]), _bits(D[rd[rd >= 0], np.nonzero(rd >= 0)[0]]))
    w.mgr.close()


# ---------------------------------------------------------------------------------------------------------------- end to end
def _labelled(w, rng, s):
    meas = np.zeros((w.n, 7)); meas[:, 6] = 1.0
    meas[:, :3] = w.p0[:, :3] + w.v0[:, :3] * DT * (s + 1) + rng.normal(0, 0.01, (w.n, 3))
    q = rng.normal(0, 0.05, (w.n, 4)) + [0, 0, 0, 1.0]
    meas[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return meas


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
        r = b.associate(_cuda(meas[perm], np.float64), DT, gate=50.0, rounds=16)
        b.step(DT, r.meas, r.has_meas)
        tb.step(DT, _cuda(meas.T, np.float64).to(tdt).contiguous(), torch.ones(n, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        assert np.array_equal(r.slot_of_det.cpu().numpy(), perm) and list(r.info.cpu().numpy())[0] == n
    x, P = w.mgr.get_state_batch(w.ids)
    tx, tP = tw.mgr.get_state_batch(tw.ids)
    assert np.array_equal(_bits(x), _bits(tx)) and np.array_equal(_bits(P), _bits(tP))
    if layout == "301shared":
        assert b.shared_axes == 1
    w.mgr.close(); tw.mgr.close()


def test_mixed_manager_through_step_sequence_all():
    """angular_rates + angular_velocities in one manager: one frame for both, scattered per batch, stepped by step_sequence_all"""
    def build():
        mgr = te.TargetManager(dtype="f64", lanes_per_target=301)
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        ws = [World("angular_rates", "f64", "301", 70, seed=3, mgr=mgr, ids=np.arange(70, dtype=np.uint32)),
              World("angular_velocities", "f64", "301", 65, seed=4, mgr=mgr, ids=np.arange(65, dtype=np.uint32) + 1000)]
        ws[1].p0[:, 2] += 4.0          # the second model's lattice above the first one's
        for w in ws:
            w.init()
        return mgr, ws
    mgr, ws = build()
    tmgr, tws = build()
    rng = np.random.default_rng(9)
    order = [te.MODEL_TYPES[w.name] for w in ws]
    bs = mgr.batches()
    ws_by_batch = [ws[order.index(b.type)] for b in bs]
    for s in range(2):
        per = [_labelled(w, rng, s) for w in ws_by_batch]
        frame = np.concatenate(per)
        perm = rng.permutation(len(frame))
        r = mgr.associate(_cuda(frame[perm], np.float64), DT, gate=50.0, rounds=16)
        mgr.step_sequence_all(DT, r.meas, r.has_meas, n_ticks=1)
        tmgr.step_sequence_all(DT, [_cuda(m.T[None], np.float64) for m in per],
                               [torch.ones((1, m.shape[0]), dtype=torch.uint8, device="cuda") for m in per], n_ticks=1)
        torch.cuda.synchronize()
        assert list(r.info.cpu().numpy())[0] == len(frame) and list(r.info.cpu().numpy())[2] == 1
        inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
        off = 0
        for i, m in enumerate(per):
            assert np.array_equal(r.det_of_slot[i].cpu().numpy()[:len(m)], inv[off:off + len(m)])
            off += len(m)
    for w, t in zip(ws, tws):
        x, P = mgr.get_state_batch(w.ids)
        tx, tP = tmgr.get_state_batch(t.ids)
        assert np.array_equal(_bits(x), _bits(tx)) and np.array_equal(_bits(P), _bits(tP))
    mgr.close(); tmgr.close()


def test_captured_graph_of_associate_and_step_replays():
    """associate -> step captured in the caller's graph: after a warm call of the same size nothing is allocated and the host is
    never waited for; two replays leave the batch bit for bit where two eager rounds leave a twin"""
    name, n = "uniform_acceleration", 130
    stream = torch.cuda.Stream()
    ws = []
    with torch.cuda.stream(stream):
        for _ in range(2):
            w = World(name, "f64", "301", n, seed=5)
            w.init()              # (the manager takes the current stream: this one)
            ws.append(w)
        rng = np.random.default_rng(10)
        frames = [_labelled(ws[0], rng, s)[rng.permutation(n)] for s in range(3)]
        det = [_cuda(f, np.float64) for f in frames]
        buf = det[0].clone()
        outs = []
        for w in ws:                  # the warm call: tick 0, eagerly, on both
            r = w.b.associate(buf, DT, gate=50.0, rounds=4)
            w.b.step(DT, r.meas, r.has_meas)
            outs.append(r)
        stream.synchronize()
        eager, graphed = ws
        for s in (1, 2):
            buf.copy_(det[s])
            r = eager.b.associate(buf, DT, gate=50.0, rounds=4, out=outs[0])
            eager.b.step(DT, r.meas, r.has_meas)
        stream.synchronize()
        want = eager.mgr.get_state_batch(eager.ids)
        g = torch.cuda.CUDAGraph()
        buf.copy_(det[1])
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            r = graphed.b.associate(buf, DT, gate=50.0, rounds=4, out=outs[1])
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
