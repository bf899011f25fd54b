"""Position covariance and time spread at the sphere crossings, on the device (target_batch_crossing_cov_dev,
target_manager_crossing_cov_dev / _batch).

Against the oracle: the scene of tests/crossing_scene.py (tests/test_crossing_scene_oracle.py asserts what is relied on here) is
filtered on both sides; the DEVICE's own delta goes to both; for every target a copy of the oracle's is stepped predict-only by
tau_i and its P^-[0:3, 0:3] is Sigma.  Tolerance: the project's own P_rel (tests/test_gpu_parity.py TOL: 1e-10 / 2e-4 of max|P^-|).
sigma_r, sigma_t and ok are held to a NumPy longdouble evaluation from the oracle's Sigma, pose_at and twist_at; the allowed error
of every row is first-order propagation of P_rel and out_atol (see _sigma_bounds).  Then what must be bit for bit: the rows form
against the dense form, the shared-axes form against the plain one, flagged uniform tiles against settled ones, the by-id form
against the batch form -- and that the call leaves the batch as it found it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import crossing_scene as cs
from conftest import HARNESS_ORDER
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

SIZES = [1, 63, 64, 65, 130]      # 130: two full separable tiles and a partial one; 13 tiles of the 6-lane dense layouts
INF = float("inf")
TMAX = 0.006      # seconds: after the scene's 12 ticks sigma_t is 3 .. 23 ms with a median near 6.5, so this bound splits the crossers
# lanes codes: full / symmetric-packed with the most lanes per target the model has
DENSE = {"uniform_velocity": (3, 103), "uniform_acceleration": (3, 103), "angular_rates": (6, 106), "angular_velocities": (6, 106)}
LAYOUTS = ["301", "301shared", "201", "full", "packed", "classes"]
CASES = [(m, d, l) for m in HARNESS_ORDER for d in ("f64", "f32") for l in LAYOUTS if not (l == "301shared" and d == "f32")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class Case:
    """one manager with the scene's n targets of a model, filtered for the scene's ticks, and the oracle's twin"""

    def __init__(self, models, name, dtype, layout, n, with_oracle=True, sequence=False, **kw):
        m = models[name]
        self.name, self.dtype, self.n, self.model = name, dtype, n, m
        self.scene = sc = cs.build(n)
        lanes = {"301": 301, "301shared": 301, "201": 201, "full": DENSE[name][0], "packed": DENSE[name][1], "classes": 301}[layout]
        self.mgr = te.TargetManager(dtype=dtype, lanes_per_target=lanes, shared_axes=(layout == "301shared"), **kw)
        self.ids = np.arange(n, dtype=np.uint32) * 3 + 11
        typ = te.MODEL_TYPES[name]
        self.cls = None
        if layout == "classes":
            self.cls = (np.arange(n) % 2).astype(np.uint32)
            # class 1 adds 1e-3 m^2 (rad^2, ...) of process noise to every state: Sigma's Q term, 6e-17 in the shipped models, becomes a
            # tenth of Sigma itself, so a row computed with the other class's Q is far outside the tolerance
            self.Q = np.stack([m["Q"], m["Q"] + 1e-3 * np.eye(m["Q"].shape[0])])
            assert self.mgr.init_batch_classes(self.ids, cs.DT, 0.0, sc["p0"], typ, self.Q, np.stack([m["R"]] * 2), np.stack([m["P"]] * 2),
                                               self.cls, sc["v0"], sc["a0"]) == n
        else:
            assert self.mgr.init_batch(self.ids, cs.DT, 0.0, sc["p0"], sc["v0"], sc["a0"], type=typ, Q=m["Q"], R=m["R"], P0=m["P"]) == n
        self.b = b = self.mgr.batches()[0]
        assert b.size == n
        if layout == "301shared":
            assert b.shared_axes == 1
        elif layout != "classes":
            assert b.shared_axes == 0
        if layout == "classes" and n > 1:
            assert b.num_classes == 2
        tdt = b.torch_dtype()
        meas = torch.from_numpy(np.ascontiguousarray(sc["meas"].transpose(0, 2, 1))).cuda().to(tdt).contiguous()     # [ticks, 7, n]
        has = _cuda(sc["has"], np.uint8)
        if sequence:      # a recorded sequence: its dense ticks look for uniform tiles from the first one
            b.step_sequence(cs.DT, meas, has, use_graph=True)
        else:
            for s in range(cs.TICKS):
                b.step(cs.DT, meas[s], has[s])
        self.orcs = None
        if with_oracle:
            if self.cls is None:
                self.orcs = [cs.oracle_batch(oracle, m, sc, dtype)]
            else:
                self.orcs = [cs.oracle_batch(oracle, m, sc, dtype, Q=self.Q[c]) for c in (0, 1)]

    def delta(self, t1):
        """the device's own query; for the models whose query never crosses, seeded horizons with the scene's fifth at -1"""
        d, _ = self.b.intersect_sphere(cs.ORIGIN, cs.RADIUS, t1=t1, want_pose=False)
        if self.name not in cs.CROSSING_MODELS:
            h = d.cpu().numpy()
            assert (h == -1.0).all()
            h = np.random.default_rng(self.n).uniform(0.1, 1.0, self.n)
            h[self.scene["miss"]] = -1.0
            d = _cuda(h, np.float64)
        return d

    def oracle_rows(self, delta, t1):
        rows = [cs.oracle_rows(o, delta, t1) for o in self.orcs]
        if self.cls is None:
            return rows[0]
        pick = lambda k: np.where(self.cls.reshape((-1,) + (1,) * (rows[0][k].ndim - 1)) == 0, rows[0][k], rows[1][k])
        return {k: pick(k) for k in rows[0]}

    def close(self):
        self.mgr.close()


def _sigma_bounds(tol, Sigma, scale, sr, st, nv, dist, vc):
    """The allowed |error| of sigma_r and sigma_t per row, to first order.  Every entry of Sigma is within E = P_rel * scale, p_c and
    v_c are within out_atol per component, so |dp|, |dv| <= sqrt(3) out_atol and the unit normal n = (p_c - o) / |p_c - o| moves by
    |dn| <= |dp| / |p_c - o|.  With q = n^T Sigma n:  |dq| <= E (|n_x| + |n_y| + |n_z|)^2 + 2 |Sigma n| |dn| <= 3 E + 2 S |dn|, S the
    sum of |Sigma|'s entries;  sigma_r = sqrt(q): |d sigma_r| = |dq| / (2 sigma_r);  with w = |n . v_c|: |dw| <= |dn| |v_c| + |dv|;
    sigma_t = sigma_r / w: |d sigma_t| <= |d sigma_r| / w + sigma_r |dw| / w^2."""
    L = np.longdouble
    E = L(tol["P_rel"]) * scale.astype(L)
    dp = dv = np.sqrt(L(3)) * L(tol["out_atol"])
    dn = dp / dist
    S = np.abs(Sigma).sum(axis=(1, 2)).astype(L)
    dq = 3 * E + 2 * S * dn
    dsr = dq / (2 * sr)
    dw = dn * np.sqrt((vc.astype(L) ** 2).sum(axis=1)) + dv
    dst = dsr / nv + sr * dw / (nv * nv)
    return dsr, dst


@pytest.mark.parametrize("name,dtype,layout", CASES)
def test_against_the_oracle(models, name, dtype, layout):
    tol = TOL[dtype]
    worst = dict(P=0.0, sr=0.0, st=0.0)
    for n in SIZES:
        c = Case(models, name, dtype, layout, n)
        now = cs.TICKS * cs.DT
        for t1 in (None, now + 0.1):
            what = "%s %s %s n %d t1 %s" % (name, dtype, layout, n, t1)
            delta = c.delta(t1)
            hd = delta.cpu().numpy()
            cand = hd >= 0
            if name in cs.CROSSING_MODELS:
                assert np.array_equal(cand, ~c.scene["miss"]), what        # who crosses is the scene's decision on the device too
            rows = c.oracle_rows(hd, t1)
            ref = None
            if cand.any():
                sr, st, nv, dist, form = cs.sigma_reference(rows["Sigma"][cand], rows["pc"][cand], rows["vc"][cand])
                dsr, dst = _sigma_bounds(tol, rows["Sigma"][cand], rows["scale"][cand], sr, st, nv, dist, rows["vc"][cand])
                assert (form > 0).all() and (nv >= 0.1).all(), what
                ref = (sr, st, dsr, dst)
                thr_r, thr_t = float(np.median(sr)), float(np.median(st))
            else:
                thr_r = thr_t = 1.0
            cov, sigma, ok = c.b.crossing_cov(delta, origin=cs.ORIGIN, radius=cs.RADIUS, t1=float("nan") if t1 is None else t1,
                                              sigma_r_max=thr_r, sigma_t_max=thr_t)
            cov2, none_s, none_ok = c.b.crossing_cov(delta, t1=float("nan") if t1 is None else t1)      # covariance only
            torch.cuda.synchronize()
            cov, sigma, ok = cov.cpu().numpy(), sigma.cpu().numpy(), ok.cpu().numpy()
            assert none_s is None and none_ok is None and np.array_equal(_bits(cov2.cpu().numpy()), _bits(cov)), what
            # non-candidates: the filler, exactly
            assert np.array_equal(_bits(cov[~cand]), _bits(np.zeros((int((~cand).sum()), 6)))), what
            assert (sigma[~cand] == -1.0).all() and (ok[~cand] == 0).all(), what
            if not cand.any():
                continue
            # Sigma against the oracle's P^-[0:3, 0:3]
            S = rows["Sigma"][cand]
            tri = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)
            err = np.abs(cov[cand] - tri) / rows["scale"][cand][:, None]
            print("%s: Sigma error %.3e of scale (allowed %.1e)" % (what, err.max(), tol["P_rel"]))
            worst["P"] = max(worst["P"], float(err.max()))
            assert np.isfinite(cov).all() and err.max() <= tol["P_rel"], what
            if layout in ("301", "301shared", "201", "classes"):          # separable: exact zeros between the axes
                assert np.array_equal(_bits(cov[cand][:, [1, 2, 4]]), _bits(np.zeros((int(cand.sum()), 3)))), what
            if layout == "301shared":                                      # one block per kind of axis: one diagonal value
                assert np.array_equal(_bits(cov[cand][:, 0]), _bits(cov[cand][:, 3])) and np.array_equal(_bits(cov[cand][:, 0]), _bits(cov[cand][:, 5])), what
            # sigma_r, sigma_t
            sr, st, dsr, dst = ref
            er, et = np.abs(sigma[cand][:, 0] - sr), np.abs(sigma[cand][:, 1] - st)
            print("%s: sigma_r error / allowed %.3e, sigma_t error / allowed %.3e" % (what, float((er / dsr).max()), float((et / dst).max())))
            worst["sr"] = max(worst["sr"], float((er / dsr).max())); worst["st"] = max(worst["st"], float((et / dst).max()))
            assert (er <= dsr).all() and (et <= dst).all(), what
            # ok against the same reference, away from the thresholds by that error
            want = (sr <= thr_r) & (st <= thr_t)
            clear = (np.abs(sr - thr_r) > dsr) & (np.abs(st - thr_t) > dst)
            assert np.array_equal(ok[cand][clear] != 0, want[clear]), what
            assert np.array_equal(ok[cand] != 0, (sigma[cand][:, 0] <= thr_r) & (sigma[cand][:, 1] <= thr_t)), what   # ... and to its own rows always
        c.close()
    print("worst over sizes: %s" % worst)


@pytest.mark.parametrize("name,dtype,layout", [("uniform_acceleration", "f64", "301shared"), ("angular_rates", "f32", "301"),
                                                ("angular_rates", "f64", "packed"), ("uniform_acceleration", "f32", "full")])
def test_rows_form_equals_dense_form(models, name, dtype, layout):
    """a shuffled slot list with -1 entries (and one slot twice): every row is the dense form's row of its slot, or the filler"""
    for n in SIZES:
        c = Case(models, name, dtype, layout, n, with_oracle=False)
        delta = c.delta(None)
        cov, sigma, ok = c.b.crossing_cov(delta, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
        rng = np.random.default_rng(n)
        slots = np.concatenate([rng.permutation(n), [-1, n - 1, -1]]).astype(np.int32)
        rng.shuffle(slots)
        hd = delta.cpu().numpy()
        drow = np.where(slots >= 0, hd[np.maximum(slots, 0)], 0.25)        # a -1 slot is skipped whatever its delta says
        cr, sr, okr = c.b.crossing_cov(_cuda(drow, np.float64), _cuda(slots, np.int32), origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
        torch.cuda.synchronize()
        cov, sigma, ok, cr, sr, okr = (t.cpu().numpy() for t in (cov, sigma, ok, cr, sr, okr))
        live = slots >= 0
        assert np.array_equal(_bits(cr[live]), _bits(cov[slots[live]])) and np.array_equal(_bits(sr[live]), _bits(sigma[slots[live]]))
        assert np.array_equal(okr[live], ok[slots[live]])
        assert not cr[~live].any() and (sr[~live] == -1.0).all() and not okr[~live].any()
        if name in cs.CROSSING_MODELS and n >= 63:
            assert 0 < ok.sum() < (~c.scene["miss"]).sum()              # the bound splits the crossers
        c.close()


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_shared_axes_form_equals_plain_form(models, name):
    for n in (65, 130):
        a, b = Case(models, name, "f64", "301shared", n, with_oracle=False), Case(models, name, "f64", "301", n, with_oracle=False)
        assert a.b.shared_axes == 1 and b.b.shared_axes == 0
        da, db = a.delta(None), b.delta(None)
        assert np.array_equal(_bits(da.cpu().numpy()), _bits(db.cpu().numpy()))
        ra = a.b.crossing_cov(da, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_r_max=0.01)
        rb = b.b.crossing_cov(db, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_r_max=0.01)
        torch.cuda.synchronize()
        for x, y in zip(ra, rb):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
        a.close(); b.close()


def _state(c):
    x, P = c.mgr.get_state_batch(c.ids)
    return _bits(x).copy(), _bits(P).copy()


@pytest.mark.parametrize("name", ["uniform_acceleration", "angular_rates"])
def test_flagged_uniform_tiles_equal_settled_ones_and_nothing_is_touched(models, name):
    """A shared-axes batch after a recorded sequence holds flagged uniform tiles (tile 0 and the partial tile 2 of 130; tile 1 is
    split by the mask).  The call reads their words from the tiles' blocks and leaves state, flags, storage form, recordings and
    rejection runs as they were; after the batch has settled its tiles (a growth of the batch does, without stepping anything) the
    same rows come out bit for bit."""
    n = 130
    c = Case(models, name, "f64", "301shared", n, with_oracle=False, sequence=True)
    b = c.b
    before = (b.shared_axes, b.uniform_tiles, b.graph_recordings)
    assert before[0] == 1 and before[1] > 0 and before[2] >= 1, before      # the precondition: there are flagged tiles
    runs = b.rejection_runs().copy()
    st = _state(c)
    delta = c.delta(None)
    rows = [t.cpu().numpy().copy() for t in b.crossing_cov(delta, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)]
    slots = _cuda(np.arange(n)[::-1].copy(), np.int32)
    listed = [t.cpu().numpy().copy() for t in b.crossing_cov(_cuda(delta.cpu().numpy()[::-1].copy(), np.float64), slots, origin=cs.ORIGIN,
                                                               radius=cs.RADIUS, sigma_t_max=TMAX)]
    found, cov_id, sig_id, ok_id = c.mgr.crossing_cov_batch(c.ids, delta.cpu().numpy(), origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
    assert (b.shared_axes, b.uniform_tiles, b.graph_recordings) == before
    assert np.array_equal(b.rejection_runs(), runs)
    after = _state(c)
    assert np.array_equal(st[0], after[0]) and np.array_equal(st[1], after[1])
    assert (b.shared_axes, b.uniform_tiles, b.graph_recordings) == before
    assert (rows[0][~c.scene["miss"]] != 0).any()
    for x, y in zip(rows, listed):
        assert np.array_equal(x.view(np.uint8), y[::-1].copy().view(np.uint8))
    # the by-id form is the batch form
    assert found == n and np.array_equal(_bits(cov_id), _bits(rows[0])) and np.array_equal(_bits(sig_id), _bits(rows[1]))
    assert np.array_equal(ok_id, rows[2] != 0)
    # settle: more targets than the batch has room for
    extra = np.arange(5000, dtype=np.uint32) + 100000
    p0 = np.tile([9.0, 9.0, 9.0, 0, 0, 0, 1.0], (len(extra), 1))
    m = models[name]
    assert c.mgr.init_batch(extra, cs.DT, 0.0, p0, type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == len(extra)
    assert b.size == n + len(extra) and b.uniform_tiles == 0 and b.shared_axes == 1
    settled = [t.cpu().numpy() for t in b.crossing_cov(delta, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)]      # rows 0 .. n-1 of the larger batch
    for x, y in zip(rows, settled):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    c.close()


def test_by_id_form_unknown_ids_and_the_queue(models):
    """ids in any order with unknown ones between them; a queued one-target step runs first, as ahead of the by-id getters"""
    name, n = "uniform_acceleration", 130
    c = Case(models, name, "f32", "301", n, with_oracle=False)
    twin = Case(models, name, "f32", "301", n, with_oracle=False)
    z = c.scene["meas"][-1][5]
    c.mgr.update(int(c.ids[5]), cs.DT, z)                          # queued, not yet run
    twin.mgr.update(int(twin.ids[5]), cs.DT, z)
    twin.mgr.synchronize()
    x_twin = twin.mgr.get_state_batch(twin.ids[5:6])               # (runs the twin's queue)
    delta = twin.delta(None)
    want = [t.cpu().numpy() for t in twin.b.crossing_cov(delta, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)]
    order = np.random.default_rng(9).permutation(n)
    ids = np.concatenate([[7], c.ids[order], [8]]).astype(np.uint32)          # 7 and 8 are nobody's id
    hd = np.concatenate([[0.5], delta.cpu().numpy()[order], [0.5]])
    found, cov, sigma, ok = c.mgr.crossing_cov_batch(ids, hd, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
    assert found == n
    assert np.array_equal(_bits(cov[1:-1]), _bits(want[0][order])) and np.array_equal(_bits(sigma[1:-1]), _bits(want[1][order]))
    assert np.array_equal(ok[1:-1], want[2][order] != 0)
    for r in (0, -1):
        assert not cov[r].any() and (sigma[r] == -1.0).all() and not ok[r]
    assert (cov[1 + int(np.flatnonzero(order == 5)[0])] != 0).any()
    c.close(); twin.close()


def test_manager_rows_behind_a_selection_and_two_shards(models):
    """tick with the query -> crossing_cov with sigma_t_max -> select_soonest with that mask -> the k rows with their covariance;
    the manager's device form serves the rows of every batch and fills the rest once; two shards (when two devices are visible)
    give the by-id rows of one"""
    n, k = 130, 16
    sc = cs.build(n)
    names = ["uniform_acceleration", "angular_rates", "uniform_velocity"]

    def population(**kw):
        mgr = te.TargetManager(dtype="f64", **kw)
        for j, name in enumerate(names):
            m = models[name]
            ids = np.arange(n, dtype=np.uint32) + 1000 * (j + 1)
            assert mgr.init_batch(ids, cs.DT, 0.0, sc["p0"], sc["v0"], sc["a0"], type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
        return mgr

    mgr = population()
    bs = mgr.batches()
    assert len(bs) == 3
    meas = [torch.from_numpy(np.ascontiguousarray(sc["meas"].transpose(0, 2, 1))).cuda().contiguous() for _ in bs]
    deltas = [torch.full((n,), -3.0, dtype=torch.float64, device="cuda") for _ in bs]
    poses = [torch.zeros((n, 7), dtype=torch.float64, device="cuda") for _ in bs]
    for s in range(cs.TICKS):
        mgr.step_sequence_all(cs.DT, [m[s:s + 1] for m in meas], query=(cs.ORIGIN, cs.RADIUS, deltas, poses), use_graph=False)
    dense = [b.crossing_cov(d, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX) for b, d in zip(bs, deltas)]
    oks = [r[2] for r in dense]
    cnt, bo, so, do, po = mgr.select_soonest((deltas, poses), ok=oks, k=k, device=True)
    cov, sigma, ok = mgr.crossing_cov(bo, so, do, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
    torch.cuda.synchronize()
    count = int(cnt.item())
    hb, hs = bo.cpu().numpy(), so.cpu().numpy()
    cov, sigma, ok = cov.cpu().numpy(), sigma.cpu().numpy(), ok.cpu().numpy()
    hok = [o.cpu().numpy() for o in oks]
    masked = sum(int(o.sum()) for o in hok)
    assert 0 < count == min(k, masked), (count, masked)
    for i in range(count):
        d = [t.cpu().numpy() for t in dense[hb[i]]]
        assert np.array_equal(_bits(cov[i]), _bits(d[0][hs[i]])) and np.array_equal(_bits(sigma[i]), _bits(d[1][hs[i]])) and ok[i] == 1
        assert sigma[i, 1] <= TMAX
    assert not cov[count:].any() and (sigma[count:] == -1.0).all() and not ok[count:].any()
    # rows of no batch of the manager (an index past its batches) and of no slot get the filler too, once
    bb = _cuda(np.array([0, 3, 1, -1, 2, 0], dtype=np.int32), np.int32)
    ss = _cuda(np.array([0, 0, -1, 0, 1, n], dtype=np.int32), np.int32)
    dd = _cuda(np.full(6, 0.5), np.float64)
    c6, s6, o6 = (t.cpu().numpy() for t in mgr.crossing_cov(bb, ss, dd, origin=cs.ORIGIN, radius=cs.RADIUS))
    assert c6[0].any() and c6[4].any() and not c6[[1, 2, 3, 5]].any() and (s6[[1, 2, 3, 5]] == -1.0).all() and not o6[[1, 2, 3, 5]].any()
    # by id over the whole manager, against the batches' dense rows
    ids = np.concatenate([b.slot_ids() for b in bs])
    alld = np.concatenate([d.cpu().numpy() for d in deltas])
    found, cid, sid, oid = mgr.crossing_cov_batch(ids, alld, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
    assert found == 3 * n
    assert np.array_equal(_bits(cid), _bits(np.concatenate([r[0].cpu().numpy() for r in dense])))
    assert np.array_equal(_bits(sid), _bits(np.concatenate([r[1].cpu().numpy() for r in dense])))
    # two shards give the rows of one (on a second device when one is visible, else both on device 0: the same host path)
    second = 1 if torch.cuda.device_count() >= 2 else 0
    two = population(devices=[0, second])
    b2 = two.batches()
    assert two.num_shards == 2 and len(b2) == 6
    m2 = []
    for i, b in enumerate(b2):          # every batch's ticks from the scene rows of the targets it holds (id = 1000 (model + 1) + row)
        rows = b.slot_ids() % 1000
        dev = "cuda:%d" % two.shard_device(two.batch_shard(i))
        m2.append(torch.from_numpy(np.ascontiguousarray(sc["meas"][:, rows, :].transpose(0, 2, 1))).to(dev).contiguous())
    for s in range(cs.TICKS):
        two.step_sequence_all(cs.DT, [m[s:s + 1] for m in m2], use_graph=False)
    f2, c2, s2, o2 = two.crossing_cov_batch(ids, alld, origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX)
    assert f2 == 3 * n and np.array_equal(_bits(c2), _bits(cid)) and np.array_equal(_bits(s2), _bits(sid)) and np.array_equal(o2, oid)
    with pytest.raises(RuntimeError, match="shards"):
        two.crossing_cov(bo, so, do)
    two.close()
    mgr.close()


def test_refusals_write_nothing(models):
    c = Case(models, "uniform_acceleration", "f64", "301", 65, with_oracle=False)
    delta = c.delta(None)
    cov = torch.full((65, 6), 7.0, dtype=torch.float64, device="cuda")
    sigma = torch.full((65, 2), 7.0, dtype=torch.float64, device="cuda")
    ok = torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    bad = [dict(origin=cs.ORIGIN, radius=0.0), dict(origin=cs.ORIGIN, radius=float("nan")), dict(origin=None, radius=1.0),
           dict(origin=cs.ORIGIN, radius=1.0, sigma_r_max=float("nan")), dict(origin=cs.ORIGIN, radius=1.0, sigma_t_max=float("nan"))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="crossing_cov"):
            c.b.crossing_cov(delta, out=(cov, sigma, ok), **kw)
    big = torch.zeros(66, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="n 66 > size 65"):
        c.b.crossing_cov(big, origin=cs.ORIGIN, radius=1.0, out=(cov, sigma, ok))
    torch.cuda.synchronize()
    assert (cov == 7.0).all() and (sigma == 7.0).all() and (ok == 7).all()
    c.close()


def _nan_records_case():
    """Child process of the test below: runs against the test build of the library (TARGET_ESTIMATION_AMD_LIB), whose
    te_test_batch_set_state reaches Batch::set_state."""
    import ctypes
    from conftest import MODEL_FILES, ROOT
    assert te.capi.LIB.endswith("_testhooks.so")
    models = {k: oracle.load_model_yaml(os.path.join(ROOT, "models", v)) for k, v in MODEL_FILES.items()}
    dp = ctypes.POINTER(ctypes.c_double)
    for name, dtype, layout in (("uniform_acceleration", "f64", "301shared"), ("angular_rates", "f32", "packed")):
        n = 130
        c = Case(models, name, dtype, layout, n, with_oracle=False)
        N = c.b.state_dim
        hook = c.b._lib.te_test_batch_set_state
        hook.argtypes, hook.restype = [ctypes.c_void_p, ctypes.c_long, dp, dp], ctypes.c_int
        x, P = np.full((n, N), np.nan), np.full((n, N, N), np.nan)
        assert hook(c.b._h, n, x.ctypes.data_as(dp), P.ctypes.data_as(dp)) == 0
        xs, Ps = c.mgr.get_state_batch(c.ids)          # (a separable layout stores no word between two axes: those entries read 0)
        assert np.isnan(xs).all() and np.isnan(Ps[:, np.arange(N), np.arange(N)]).all()
        d = np.full(n, -1.0); d[::3] = np.nan; d[1::7] = -0.5; d[5] = -np.inf
        cov, sigma, ok = (t.cpu().numpy() for t in c.b.crossing_cov(_cuda(d, np.float64), origin=cs.ORIGIN, radius=cs.RADIUS))
        assert np.array_equal(_bits(cov), _bits(np.zeros((n, 6)))) and (sigma == -1.0).all() and not ok.any(), name
        d[4] = 0.5          # one candidate: its row reads the records, which are NaN
        cov, sigma, ok = (t.cpu().numpy() for t in c.b.crossing_cov(_cuda(d, np.float64), origin=cs.ORIGIN, radius=cs.RADIUS))
        assert np.isnan(cov[4, [0, 3, 5]]).all() and np.isnan(sigma[4]).all() and ok[4] == 0 and not cov[np.arange(n) != 4].any(), name
        c.close()
    print("nan records case ok")


def test_non_candidates_read_no_record():
    """an all -1 (NaN, negative) delta returns the filler even over a batch whose records were just set to NaN through set_state"""
    from target_estimation_amd import _build
    lib = _build.build_testhooks()
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TARGET_ESTIMATION_AMD_LIB=lib, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_crossing_cov as t; t._nan_records_case()"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "nan records case ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_captured_in_a_graph_behind_a_tick_and_a_selection(models):
    """one-tick sequence with the query -> dense crossing_cov (the mask) -> select_soonest_dev -> the manager's rows form, captured
    once on the manager's stream and replayed twice, against the same calls made eagerly twice on a twin: the same bits"""
    n, k, name = 130, 8, "uniform_acceleration"
    sc = cs.build(n)
    m = models[name]

    def fresh():
        mgr = te.TargetManager(dtype="f64")
        ids = np.arange(n, dtype=np.uint32) + 1
        assert mgr.init_batch(ids, cs.DT, 0.0, sc["p0"], sc["v0"], sc["a0"], type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
        meas = torch.from_numpy(np.ascontiguousarray(sc["meas"].transpose(0, 2, 1))).cuda().contiguous()
        buf = dict(meas=meas, delta=[torch.full((n,), -3.0, dtype=torch.float64, device="cuda")], pose=[torch.zeros((n, 7), dtype=torch.float64, device="cuda")],
                   dense=(torch.zeros((n, 6), dtype=torch.float64, device="cuda"), torch.zeros((n, 2), dtype=torch.float64, device="cuda"),
                          torch.zeros(n, dtype=torch.uint8, device="cuda")),
                   sel=(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(k, dtype=torch.int32, device="cuda"),
                        torch.zeros(k, dtype=torch.int32, device="cuda"), torch.zeros(k, dtype=torch.float64, device="cuda"),
                        torch.zeros((k, 7), dtype=torch.float64, device="cuda")),
                   rows=(torch.zeros((k, 6), dtype=torch.float64, device="cuda"), torch.zeros((k, 2), dtype=torch.float64, device="cuda"),
                         torch.zeros(k, dtype=torch.uint8, device="cuda")))
        return mgr, buf

    def chain(mgr, buf, s):
        b = mgr.batches()[0]
        mgr.step_sequence_all(cs.DT, [buf["meas"][s:s + 1]], query=(cs.ORIGIN, cs.RADIUS, buf["delta"], buf["pose"]), use_graph=False)
        b.crossing_cov(buf["delta"][0], origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX, out=buf["dense"])
        mgr.select_soonest((buf["delta"], buf["pose"]), ok=[buf["dense"][2]], k=k, device=True, out=buf["sel"])
        mgr.crossing_cov(buf["sel"][1], buf["sel"][2], buf["sel"][3], origin=cs.ORIGIN, radius=cs.RADIUS, sigma_t_max=TMAX, out=buf["rows"])

    def result(buf):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in buf["sel"] + buf["rows"] + buf["dense"]]

    warm = cs.TICKS - 2
    eager, ebuf = fresh()
    for s in range(warm):
        chain(eager, ebuf, s)          # (warm: the shard's selection scratch is allocated by the first call)
    chain(eager, ebuf, warm); chain(eager, ebuf, warm)
    want = result(ebuf)
    assert int(want[0][0]) > 0

    mgr, buf = fresh()
    for s in range(warm):
        chain(mgr, buf, s)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    mgr.set_stream(stream.cuda_stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        chain(mgr, buf, warm)
    g.replay(); g.replay()
    got = result(buf)
    for x, y in zip(want, got):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    mgr.set_stream(None)
    eager.close(); mgr.close()
