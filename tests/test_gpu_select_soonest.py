"""The k soonest sphere crossings selected on the device (target_batch_select_soonest[_dev], target_manager_select_soonest[_dev]).

The yardstick is NumPy on the arrays read back:
    cand = flatnonzero(ok & (d >= lo) & (d <= hi)); sel = cand[lexsort((cand, d[cand]))][:k]
(the manager form has the batch index as the middle key).  Slots, delta bits and pose rows must be EQUAL.  First on synthetic device
arrays attached to small batches -- every size, k, tie, special value, mask and refusal of the contract, and the first stage's grid
shaped by TE_SELECT_SOONEST_MAX_WGS -- then on the real path: ticks with the query, the convergence gate's mask, one and three
shards, and a shared-axes batch with uniform tiles, which the selection must leave alone."""
import os

import numpy as np
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from target_estimation_amd import capi  # noqa: E402

DT = 0.004
INF = float("inf")
CHUNK = 256          # entries a workgroup looks at per round (csrc/select_soonest_plan.hpp, kSoonestChunk)
KNOB = "TE_SELECT_SOONEST_MAX_WGS"


def _manager(n, max_wgs=None, **kw):
    """a uniform_velocity manager with n targets (its one batch has size n; n == 0: created and erased); the knob is read at creation"""
    old = os.environ.pop(KNOB, None)
    if max_wgs is not None:
        os.environ[KNOB] = str(max_wgs)
    try:
        mgr = te.TargetManager(model_path("uniform_velocity"), **kw)
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old
    m = max(n, 1)
    ids = np.arange(m, dtype=np.uint32) * 2 + 5
    p0 = np.tile([0, 0, 0, 0, 0, 0, 1.0], (m, 1))
    assert mgr.init_batch(ids, DT, 0.0, p0) == m
    if n == 0:
        assert mgr.erase_batch(ids) == 1
    b = mgr.batches()[0]
    assert b.size == n
    return mgr, b


def _ref(d, ok, lo, hi, k, batch=None):
    okm = np.ones(len(d), bool) if ok is None else np.asarray(ok) != 0
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(okm & (d >= lo) & (d <= hi))
    keys = (cand, d[cand]) if batch is None else (cand, batch[cand], d[cand])
    return cand[np.lexsort(keys)][:k]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


FILL_POSE = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _assert_rows(sel, d, pose, count, slots, delta, prow, k, what):
    assert count == len(sel), (what, count, len(sel))
    assert np.array_equal(slots[:count], sel), (what, slots[:count], sel)
    assert np.array_equal(_bits(delta[:count]), _bits(d[sel])), what
    assert (slots[count:k] == -1).all() and (delta[count:k] == -1.0).all(), what
    if pose is not None:
        assert np.array_equal(_bits(prow[:count]), _bits(pose[sel])), what
        assert np.array_equal(prow[count:k], np.tile(FILL_POSE, (k - count, 1))), what


def _check(b, d, pose=None, ok=None, k=8, lo=0.0, hi=INF, what=""):
    """both forms of the batch call against NumPy"""
    n = b.size
    assert len(d) == n
    def dev(a, dtype):      # (an empty tensor has no address: an empty batch's arrays still hold one element, as an allocation would)
        a = np.ascontiguousarray(a, dtype=dtype)
        return torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], dtype)).cuda()
    dd = dev(d, np.float64)
    pd = None if pose is None else dev(pose, np.float64)
    od = None if ok is None else dev(ok, np.uint8)
    sel = _ref(d, ok, lo, hi, k)
    cnt, so, do, po = b.select_soonest(dd, pd, od, k=k, window=(lo, hi), device=True)
    torch.cuda.synchronize()
    _assert_rows(sel, d, pose, int(cnt.item()), so.cpu().numpy(), do.cpu().numpy(), None if po is None else po.cpu().numpy(), k, what + " dev")
    count, ids, slots, delta, prow = b.select_soonest(dd, pd, od, k=k, window=(lo, hi))
    _assert_rows(sel, d, pose, count, slots, delta, prow, k, what + " host")
    sid = b.slot_ids()
    assert np.array_equal(ids[:count], sid[sel]) and (ids[count:k] == 0xFFFFFFFF).all(), what
    return sel


def _data(n, seed, special=True):
    """deltas as a query leaves them -- crossings, many -1 -- plus, with special, NaN, +inf, both zeros and bit-equal runs"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, 10.0, n)
    d[rng.random(n) < 0.3] = -1.0
    if special and n >= 8:
        j = rng.permutation(n)
        d[j[0]] = np.nan; d[j[1]] = INF; d[j[2]] = -0.0; d[j[3]] = 0.0; d[j[4]] = -0.0
        d[j[5:5 + n // 6]] = 2.5          # a run of bit-equal deltas, scattered over the slots
    pose = rng.normal(size=(n, 7))
    return d, pose


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes_and_k(n):
    mgr, b = _manager(n)
    d, pose = _data(n, 100 + n)
    ok = (np.random.default_rng(n).random(n) < 0.7).astype(np.uint8)
    for k in (1, 2, 64, 256):          # k > n and k > candidates among them
        _check(b, d, pose, None, k, what="n %d k %d" % (n, k))
        _check(b, d, None, ok, k, what="n %d k %d masked, no gather" % (n, k))
        _check(b, d, pose, ok, k, lo=1.0, hi=7.5, what="n %d k %d window" % (n, k))
    mgr.close()


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_grid_shapes(cap):
    """the knob caps the first stage: several rounds per workgroup, an exact multiple of the grid's share, that multiple plus one"""
    for n in (CHUNK * cap * 3 + 17, CHUNK * cap * 2, CHUNK * cap * 2 + 1):
        mgr, b = _manager(n, max_wgs=cap)
        d, pose = _data(n, 7 * n + cap)
        ok = (np.random.default_rng(n + 1).random(n) < 0.5).astype(np.uint8)
        for k in (1, 64, 256):
            _check(b, d, pose, None, k, what="cap %d n %d k %d" % (cap, n, k))
            _check(b, d, pose, ok, k, lo=0.5, hi=9.0, what="cap %d n %d k %d masked" % (cap, n, k))
        # every entry a candidate: every round fills the collected half
        _check(b, np.random.default_rng(3).uniform(0, 1, n), None, None, 256, what="cap %d n %d all candidates" % (cap, n))
        mgr.close()


def test_more_workgroups_than_rounds_and_ties_across_them():
    """n = 1000 with the default cap: four workgroups of one round each.  A block of bit-equal deltas straddles position k, its slots
    spread over all four ranges: the smaller slots win."""
    n = 1000
    mgr, b = _manager(n)
    rng = np.random.default_rng(5)
    d = rng.uniform(5.0, 6.0, n)
    tied = np.sort(rng.choice(n, 400, replace=False))
    d[tied] = 1.0
    early = rng.choice(np.setdiff1d(np.arange(n), tied), 5, replace=False)
    d[early] = 0.5
    pose = rng.normal(size=(n, 7))
    assert len({int(t) // CHUNK for t in tied}) == 4
    for k in (2, 8, 64, 256):
        sel = _check(b, d, pose, None, k, what="ties k %d" % k)
        if k > 5:
            assert np.array_equal(np.sort(sel[5:]), tied[:k - 5])
    # all of them tied: slot order
    sel = _check(b, np.full(n, 3.25), pose, None, 256, what="all tied")
    assert np.array_equal(sel, np.arange(256))
    mgr.close()


def test_special_values_and_windows():
    n = 300
    mgr, b = _manager(n)
    rng = np.random.default_rng(9)
    # no candidate at all
    _check(b, np.full(n, -1.0), rng.normal(size=(n, 7)), None, 8, what="all -1")
    _check(b, np.full(n, np.nan), None, None, 8, what="all NaN")
    # -0.0 next to 0.0: equal as doubles, the slot decides, and the row carries the input's own bits
    d = rng.uniform(1.0, 2.0, n)
    d[10] = 0.0; d[11] = -0.0; d[200] = -0.0; d[201] = 0.0
    sel = _check(b, d, None, None, 4, what="zeros")
    assert list(sel) == [10, 11, 200, 201]
    # NaN and +inf: +inf is a candidate of an open window and comes last, NaN never is one
    d = rng.uniform(1.0, 2.0, n)
    d[100:] = -1.0
    d[3] = np.nan; d[4] = INF; d[250] = INF; d[5] = -1.0
    sel = _check(b, d, None, None, 256, hi=INF, what="inf")
    assert len(sel) == 99 and list(sel[-2:]) == [4, 250]
    sel = _check(b, d, None, None, 256, hi=1e300, what="finite hi")
    assert len(sel) == 97
    # a window that cuts inside the data: the entries equal to delta_lo and to delta_hi are both in
    d = np.linspace(0.0, 29.9, n)
    lo, hi = float(d[100]), float(d[120])
    sel = _check(b, d, None, None, 64, lo=lo, hi=hi, what="window")
    assert list(sel) == list(range(100, 121))
    sel = _check(b, d, None, None, 5, lo=lo, hi=lo, what="one-point window")
    assert list(sel) == [100]
    # masks: none, all zero, random; a bool tensor's bytes count too
    d, pose = _data(n, 77)
    _check(b, d, pose, np.zeros(n, np.uint8), 8, what="mask all zero")
    _check(b, d, pose, (rng.random(n) < 0.5).astype(np.uint8) * 255, 64, what="mask random")
    mgr.close()


def test_refusals_leave_everything_untouched():
    n = 100
    mgr, b = _manager(n)
    d, pose = _data(n, 1)
    dd, pd = torch.from_numpy(d).cuda(), torch.from_numpy(pose).cuda()

    def outs():
        return (torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((256,), -7, dtype=torch.int32, device="cuda"),
                torch.full((256,), -7.0, dtype=torch.float64, device="cuda"), torch.full((256, 7), -7.0, dtype=torch.float64, device="cuda"))

    nan = float("nan")
    cases = [  # (delta, pose, k, window, which outputs are NULL, with pose_out)
        (dd, pd, 0, (0.0, INF), (), True), (dd, pd, 257, (0.0, INF), (), True), (dd, pd, -3, (0.0, INF), (), True),
        (dd, pd, 8, (-1.0, INF), (), True), (dd, pd, 8, (nan, INF), (), True),
        (dd, pd, 8, (2.0, 1.0), (), True), (dd, pd, 8, (0.0, nan), (), True),
        (None, pd, 8, (0.0, INF), (), True),
        (dd, pd, 8, (0.0, INF), (0,), True), (dd, pd, 8, (0.0, INF), (1,), True), (dd, pd, 8, (0.0, INF), (2,), True),
        (dd, None, 8, (0.0, INF), (), True),      # pose_out without pose
        (dd, pd, 8, (0.0, INF), (3,), True),      # pose without pose_out
    ]
    rec = b.graph_recordings
    for delta, p, k, window, nulls, _ in cases:
        o = list(outs())
        keep = [t.clone() for t in o]
        for j in nulls:
            o[j] = None
        with pytest.raises(RuntimeError, match="select_soonest"):
            b.select_soonest(delta, p, None, k=k, window=window, device=True, out=tuple(o))
        assert b"select_soonest" in capi.lib().target_manager_last_error()
        torch.cuda.synchronize()
        for t, was in zip(o, keep):
            assert t is None or torch.equal(t, was)
        # the host form refuses the same (its id / slot / delta arrays in place of count / slot / delta)
        h = [np.full(256, 7, np.uint32), np.full(256, -7, np.int32), np.full(256, -7.0), np.full((256, 7), -7.0)]
        hk = [a.copy() for a in h]
        for j in nulls:
            h[j] = None
        with pytest.raises(RuntimeError, match="select_soonest"):
            b.select_soonest(delta, p, None, k=k, window=window, out=tuple(h))
        for a, was in zip(h, hk):
            assert a is None or np.array_equal(a, was)
    assert b.graph_recordings == rec and b.size == n
    # the manager forms: the wrong number of batches, a gather from a batch without pose rows, a NULL output, several shards
    with pytest.raises(RuntimeError, match="one description per batch"):
        mgr.select_soonest(([dd, dd], [pd, pd]))
    with pytest.raises(RuntimeError, match="nothing to gather from"):
        mgr.select_soonest(([dd], [None]), out=(np.zeros(8, np.uint32), np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8), np.zeros((8, 7))))
    with pytest.raises(RuntimeError, match="every output"):
        mgr.select_soonest(([dd], None), out=(np.zeros(8, np.uint32), None, np.zeros(8, np.int32), np.zeros(8), None))
    with pytest.raises(RuntimeError, match="k must be"):
        mgr.select_soonest(([dd], [pd]), k=300)
    _check(b, d, pose, None, 8, what="after the refusals")
    mgr.close()
    sh = te.TargetManager(model_path("uniform_velocity"), devices=[0, 0])
    with pytest.raises(RuntimeError, match="no single device"):
        sh.select_soonest(([], []), device=True)
    sh.close()


def test_back_to_back_calls_share_the_scratch_in_stream_order():
    n = 3000
    mgr, b = _manager(n, max_wgs=4)
    d1, p1 = _data(n, 21)
    d2, p2 = _data(n, 22)
    t1, t2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()
    q1, q2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    torch.cuda.synchronize()
    r1 = b.select_soonest(t1, q1, None, k=64, device=True)
    r2 = b.select_soonest(t2, q2, None, k=256, window=(1.0, 8.0), device=True)
    torch.cuda.synchronize()
    for (cnt, so, do, po), d, p, k, lo, hi in ((r1, d1, p1, 64, 0.0, INF), (r2, d2, p2, 256, 1.0, 8.0)):
        _assert_rows(_ref(d, None, lo, hi, k), d, p, int(cnt.item()), so.cpu().numpy(), do.cpu().numpy(), po.cpu().numpy(), k, "back to back")
    mgr.close()


# ---- the real path ------------------------------------------------------------------------------------------------------------
POP = [("uniform_acceleration", 1000, 0), ("angular_rates", 1000, 5000), ("uniform_velocity", 300, 10000)]
ORIGIN, RADIUS = (0.0, 0.0, 0.0), 5.0
TICKS = 4
# By id, so that a target sees the same stream whichever shard and slot it lands in.  The query reports the leftmost real root of
# |p + v d + a d^2 / 2 - origin| = radius and only if it is not negative, so a crossing needs a target outside the sphere that closes
# in while it DECELERATES (one that accelerates towards the sphere has, as a parabola, also crossed it in the past and reports -1):
# a start 8 .. 15 from the origin, 24 .. 36 per second towards it, 10 per second^2 away from it, created with that motion, plus noise.
_rng = np.random.default_rng(31)
_dir = _rng.normal(size=(11000, 3))
_dir /= np.linalg.norm(_dir, axis=1, keepdims=True)
START = _dir * _rng.uniform(8.0, 15.0, (11000, 1))
VEL = -_dir * _rng.uniform(24.0, 36.0, (11000, 1))
ACC = _dir * 10.0
NOISE = np.random.default_rng(8).normal(scale=0.02, size=(11000, 4 * TICKS, 3))


def _population(models, dtype, devices=None):
    mgr = te.TargetManager(dtype=dtype, devices=devices)
    for name, n, base in POP:
        m = models[name]
        ids = np.arange(n, dtype=np.uint32) + base
        p0 = np.concatenate([START[ids], np.tile([0, 0, 0, 1.0], (n, 1))], 1)
        v0 = np.concatenate([VEL[ids], np.zeros((n, 3))], 1)
        a0 = np.concatenate([ACC[ids], np.zeros((n, 3))], 1)
        assert mgr.init_batch(ids, DT, 0.0, p0, v0=v0, a0=a0, type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
    return mgr


def _tick_and_select(mgr, dtype, k, window, with_mask, first=0):
    """TICKS ticks with the query and the gate, then the selections; returns the manager rows as (id, delta bits, pose) and checks
    the batch form and the manager form against NumPy on the arrays read back"""
    tdt = torch.float64 if dtype == "f64" else torch.float32
    bs = mgr.batches()
    meas, deltas, poses = [], [], []
    for b in bs:
        ids = b.slot_ids()
        t = np.zeros((TICKS, 7, len(ids)))
        at = (DT * (first + np.arange(1, TICKS + 1)))[:, None, None]
        t[:, :3, :] = NOISE[ids, first:first + TICKS].transpose(1, 2, 0) + START[ids].T[None] + VEL[ids].T[None] * at + 0.5 * ACC[ids].T[None] * at * at
        t[:, 6, :] = 1.0
        meas.append(torch.tensor(t, dtype=tdt, device="cuda"))
        deltas.append(torch.full((b.size,), -3.0, dtype=torch.float64, device="cuda"))
        poses.append(torch.zeros((b.size, 7), dtype=torch.float64, device="cuda"))
    # The gate's mask.  Its first position error is the distance from the gate's initial pose [0 0 0] to the sphere, i.e. RADIUS, so the
    # window is 2 ticks: from the third tick on the average holds differences of consecutive crossings only.  The last tick's threshold
    # is the median of the averages one tick earlier (the same number on every manager that holds these targets): a proper subset.
    masks, pos_th = [], 1e9
    for s in range(TICKS):
        mgr.step_sequence_all(DT, [m[s:s + 1] for m in meas], query=(ORIGIN, RADIUS, deltas, poses), use_graph=False)
        res = [b.gate_update(d, p, pos_th, 1e9, filters_length=2) if b.size else None for b, d, p in zip(bs, deltas, poses)]
        masks = [None if r is None else r[0] for r in res]
        if s == TICKS - 2:
            torch.cuda.synchronize()
            pos_th = float(np.median(np.concatenate([r[1].cpu().numpy()[d.cpu().numpy() >= 0, 0] for r, d in zip(res, deltas) if r is not None])))
    mgr.synchronize()
    torch.cuda.synchronize()
    ok = masks if with_mask else None
    hd = [d.cpu().numpy() for d in deltas]
    hp = [p.cpu().numpy() for p in poses]
    hok = [None if (ok is None or o is None) else o.cpu().numpy() for o in (masks if ok is not None else [None] * len(bs))]
    sids = [b.slot_ids() for b in bs]
    lo, hi = window
    for i, b in enumerate(bs):       # the batch form
        if b.size == 0:
            continue
        sel = _ref(hd[i], hok[i], lo, hi, k)
        count, ids, slots, delta, prow = b.select_soonest(deltas[i], poses[i], None if ok is None else ok[i], k=k, window=window)
        _assert_rows(sel, hd[i], hp[i], count, slots, delta, prow, k, "batch %d" % i)
        assert np.array_equal(ids[:count], sids[i][sel])
    # the manager form: (delta, batch, slot)
    alld = np.concatenate(hd)
    allb = np.concatenate([np.full(len(d), i) for i, d in enumerate(hd)])
    alls = np.concatenate([np.arange(len(d)) for d in hd])
    allok = None if ok is None else np.concatenate([np.ones(len(d), np.uint8) if o is None else o for d, o in zip(hd, hok)])
    sel = _ref(alld, allok, lo, hi, k, batch=allb)
    count, ids, bo, so, do, po = mgr.select_soonest((ORIGIN, RADIUS, deltas, poses), ok=ok, k=k, window=window)
    assert count == len(sel)
    assert np.array_equal(bo[:count], allb[sel]) and np.array_equal(so[:count], alls[sel])
    assert np.array_equal(_bits(do[:count]), _bits(alld[sel]))
    assert np.array_equal(_bits(po[:count]), _bits(np.concatenate(hp)[sel]))
    assert np.array_equal(ids[:count], np.concatenate(sids)[sel])
    assert (bo[count:] == -1).all() and (so[count:] == -1).all() and (do[count:] == -1).all() and (ids[count:] == 0xFFFFFFFF).all()
    if mgr.num_shards == 1:        # the device form of the manager call
        cnt, bd, sd, dd, pd = mgr.select_soonest((deltas, poses), ok=ok, k=k, window=window, device=True)
        torch.cuda.synchronize()
        assert int(cnt.item()) == count and np.array_equal(bd.cpu().numpy(), bo) and np.array_equal(sd.cpu().numpy(), so)
        assert np.array_equal(_bits(dd.cpu().numpy()), _bits(do)) and np.array_equal(_bits(pd.cpu().numpy()), _bits(po))
    stats = dict(candidates=int((alld >= 0).sum()), masked=None if allok is None else int(((alld >= 0) & (allok != 0)).sum()))
    if with_mask:        # the mask is a proper, non-empty subset of the crossings, and rows were selected through it
        assert 0 < stats["masked"] < stats["candidates"], stats
        assert count > 0
    return count, ids[:count].copy(), _bits(do[:count]).copy(), _bits(po[:count]).copy(), stats


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_real_path_one_shard(models, dtype):
    mgr = _population(models, dtype)
    count, ids, dbits, pbits, stats = _tick_and_select(mgr, dtype, 8, (0.0, INF), False)
    assert count == 8 and stats["candidates"] >= 64        # enough crossings for every k used here; uniform_velocity never crosses
    assert (ids < 10000).all()
    mgr2 = _population(models, dtype)
    c2 = _tick_and_select(mgr2, dtype, 64, (0.0, INF), True)
    print("f%s: candidates %d, converged %s, selected %d" % (dtype[1:], stats["candidates"], c2[4]["masked"], c2[0]))
    mgr3 = _population(models, dtype)
    srt = np.sort(np.frombuffer(dbits.tobytes(), dtype=np.float64))
    _tick_and_select(mgr3, dtype, 64, (float(srt[2]), float(srt[6])), False)      # a window that cuts inside, its ends included
    for m in (mgr, mgr2, mgr3):
        m.close()


def test_real_path_three_shards_select_the_same_targets(models):
    one = _population(models, "f64")
    three = _population(models, "f64", devices=[0, 0, 0])
    assert three.num_shards == 3 and len(three.batches()) == 9
    for call, (k, mask) in enumerate(((8, False), (64, True))):
        a = _tick_and_select(one, "f64", k, (0.0, INF), mask, first=call * TICKS)
        b = _tick_and_select(three, "f64", k, (0.0, INF), mask, first=call * TICKS)
        assert a[0] == b[0] and a[0] > 0 and (mask or a[0] == k)
        assert len(np.unique(a[2])) == a[0]   # no ties in this population: the rows are the same whatever batch an id landed in
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    one.close(); three.close()


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one_shard", "three_shards"])
def test_manager_form_with_a_mask_per_batch(models, devices):
    """synthetic arrays on every batch of a manager, a different random mask per batch (one batch without a mask, one skipped in a
    second call): a mask handed to the wrong batch, or offset across shards, selects other rows than NumPy does"""
    mgr = _population(models, "f64", devices)
    bs = mgr.batches()
    nb = len(bs)
    assert nb == (3 if devices is None else 9)
    rng = np.random.default_rng(41 + nb)
    hd, hp, hok = [], [], []
    for i, b in enumerate(bs):
        d = rng.uniform(0.0, 4.0, b.size)
        d[rng.random(b.size) < 0.3] = -1.0
        d[rng.random(b.size) < 0.2] = 1.5            # ties within and across the batches
        hd.append(d)
        hp.append(rng.normal(size=(b.size, 7)))
        hok.append(None if i == 1 else (rng.random(b.size) < 0.2 + 0.08 * i).astype(np.uint8))
    deltas = [torch.from_numpy(d).cuda() for d in hd]
    poses = [torch.from_numpy(p).cuda() for p in hp]
    oks = [None if o is None else torch.from_numpy(o).cuda() for o in hok]
    sids = np.concatenate([b.slot_ids() for b in bs])
    allp = np.concatenate(hp)
    alls = np.concatenate([np.arange(len(d)) for d in hd])
    for skip in (None, 0):
        dl = [None if i == skip else t for i, t in enumerate(deltas)]
        alld = np.concatenate([np.full(len(d), -1.0) if i == skip else d for i, d in enumerate(hd)])
        allb = np.concatenate([np.full(len(d), i) for i, d in enumerate(hd)])
        allok = np.concatenate([np.ones(len(d), np.uint8) if o is None else o for d, o in zip(hd, hok)])
        for k, (lo, hi) in ((8, (0.0, INF)), (256, (0.5, 3.0)), (64, (1.5, 1.5))):
            sel = _ref(alld, allok, lo, hi, k, batch=allb)
            assert len(sel) > 0
            count, ids, bo, so, do, po = mgr.select_soonest((dl, poses), ok=oks, k=k, window=(lo, hi))
            assert count == len(sel)
            assert np.array_equal(bo[:count], allb[sel]) and np.array_equal(so[:count], alls[sel]) and np.array_equal(ids[:count], sids[sel])
            assert np.array_equal(_bits(do[:count]), _bits(alld[sel])) and np.array_equal(_bits(po[:count]), _bits(allp[sel]))
            assert (bo[count:] == -1).all() and (so[count:] == -1).all() and (do[count:] == -1).all()
            if devices is None:
                cnt, bd, sd, dd, pd = mgr.select_soonest((dl, poses), ok=oks, k=k, window=(lo, hi), device=True)
                torch.cuda.synchronize()
                assert int(cnt.item()) == count and np.array_equal(bd.cpu().numpy(), bo) and np.array_equal(sd.cpu().numpy(), so)
                assert np.array_equal(_bits(dd.cpu().numpy()), _bits(do)) and np.array_equal(_bits(pd.cpu().numpy()), _bits(po))
    mgr.close()


def test_selection_leaves_the_storage_form_alone(models):
    """a shared-axes batch with flagged uniform tiles and a recorded sequence: the selection settles, demotes and drops nothing"""
    name, n = "uniform_acceleration", 200
    m = models[name]
    mgr = te.TargetManager(dtype="f64")
    ids = np.arange(n, dtype=np.uint32) + 1
    p0 = np.tile([8.0, -6.0, 5.0, 0, 0, 0, 1.0], (n, 1))          # created in bulk with equal state, outside the sphere: bit-equal deltas
    start = np.array([8.0, -6.0, 5.0])
    u = start / np.linalg.norm(start)
    v0 = np.tile(np.concatenate([-30.0 * u, np.zeros(3)]), (n, 1))      # closing in on the origin, decelerating (see the real path below)
    a0 = np.tile(np.concatenate([20.0 * u, np.zeros(3)]), (n, 1))
    assert mgr.init_batch(ids, DT, 0.0, p0, v0=v0, a0=a0, type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
    b = mgr.batches()[0]
    meas = torch.zeros((6, 7, n), dtype=torch.float64, device="cuda")
    at = DT * np.arange(1, 7)[:, None]
    meas[:, :3, :] = torch.from_numpy(start[None] - 30.0 * u[None] * at + 10.0 * u[None] * at * at).cuda()[:, :, None]
    meas[:, 6, :] = 1.0
    b.step_sequence(DT, meas, use_graph=True)
    delta, pose = b.intersect_sphere(ORIGIN, RADIUS)
    torch.cuda.synchronize()
    before = (b.shared_axes, b.uniform_tiles, b.graph_recordings)
    assert before[0] == 1 and before[1] == (n + 63) // 64 and before[2] >= 1
    d = delta.cpu().numpy()
    assert (d > 0).all() and len(np.unique(_bits(d))) == 1
    sel = _check(b, d, pose.cpu().numpy(), None, 8, what="shared axes")
    assert list(sel) == list(range(8))                                # ties: the smaller slots
    count = mgr.select_soonest(([delta], [pose]), k=64)[0]
    assert count == 64
    assert (b.shared_axes, b.uniform_tiles, b.graph_recordings) == before
    mgr.close()
