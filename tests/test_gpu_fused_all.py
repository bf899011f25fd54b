"""One launch for a temporally fused replay of a whole manager (target_manager_step_fused_all / _dt;
TargetManager.step_fused_all in manager.py): for every batch it must leave, bit for bit, what the per-batch fused calls
(Batch.step_fused(..., innov=, gate=, reacquire=)) leave when they are made in batch order on a second manager built from the same
inputs -- state, covariance, times, measurement counters, rejection runs, every NIS row, innovation block and event row.

The streams are tests/reacquire_ref.py's (203 targets, 20 ticks, masked ticks, +0.5 m outliers, yaw spikes, the jump at tick 8),
cut or tiled to each part's size; ld = n + 13, the padding NaN / PAD and never written.  One case steps the oracle per model."""
import ctypes as C

import numpy as np
import pytest

import gate_ref
import innov_stream_ref
import oracle
import reacquire_ref as rq
from test_gpu_parity import check_state

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from target_estimation_amd import capi  # noqa: E402
from target_estimation_amd.manager import _innov_stream, _reacquire  # noqa: E402
from test_gpu_innov_stream import _bufs, _read, _soa  # noqa: E402
from test_gpu_reacquire import PAD, _events, _read_events  # noqa: E402

DT = rq.DT
AR, AV, UA, UV = "angular_rates", "angular_velocities", "uniform_acceleration", "uniform_velocity"
# batch order differs from the kernel's part order (AR, AV, UA, UV) on purpose; partial wavefronts and every part boundary
FOUR = [(UV, 130), (AR, 65), (UA, 1), (AV, 64)]
TWO = [(UA, 70), (AR, 65)]   # no AV batch: an absent model in the middle of the grid


def _part(name, n, dtype, ticks, nan_target=False, clean=False):
    """the shared stream of `name`, columns repeated / cut to n targets, `ticks` ticks; nan_target (for a gated part: without a gate a
    NaN measurement is the state's): the last target gets NaN measurements on ticks 2-3; clean: the stream before its outliers"""
    if clean:
        p0, meas, mask, _ = innov_stream_ref.stream_and_reference(name, gate_ref.N, gate_ref.TICKS, gate_ref.SEED)
    else:
        p0, meas, mask, _, _ = rq.stream(name)
    cols = np.arange(n) % rq.N
    p0, meas, mask = p0[cols].copy(), meas[:ticks, cols].copy(), mask[:ticks, cols].copy()
    if nan_target and n > 1 and ticks > 3:
        mask[2:4, n - 1] = 1
        meas[2:4, n - 1, 0] = np.nan
    ld = n + 13
    return dict(name=name, n=n, m=gate_ref.m_of(name), ld=ld, p0=p0, meas=meas, mask=mask, soa=_soa(meas, dtype, ld),
                has=torch.from_numpy(mask.copy()).cuda())


def _manager(models, parts, dtype, shared=False, devices=None, lanes=301, two_classes_in=None):
    mgr = te.TargetManager(dtype=dtype, lanes_per_target=lanes, shared_axes=shared, devices=devices)
    base = 0
    for p in parts:
        mdl = models[p["name"]]
        p["ids"] = np.arange(p["n"], dtype=np.uint32) * 3 + 1 + base
        base += 3 * p["n"] + 7
        if two_classes_in == p["name"]:
            Q, R, P0 = (np.asarray(mdl[k], float) for k in ("Q", "R", "P"))
            assert mgr.init_batch_classes(p["ids"], DT, 0.0, p["p0"], mdl["model"], np.stack([Q, 2.0 * Q]), np.stack([R, 1.5 * R]), np.stack([P0, P0]),
                                          (np.arange(p["n"]) % 2).astype(np.uint32)) == p["n"]
        else:
            assert mgr.init_batch(p["ids"], DT, 0.0, p["p0"], type=mdl["model"], Q=mdl["Q"], R=mdl["R"], P0=mdl["P"]) == p["n"]
    assert len(mgr.batches()) == len(parts)
    return mgr


def _streams(parts, blocks, with_innov, with_events):
    """per part: (nis, nu) buffers or None, event rows or None"""
    bufs = [_bufs(blocks, p["m"], p["ld"]) if w else None for p, w in zip(parts, with_innov)]
    evs = [_events(blocks, p["ld"]) if w else None for p, w in zip(parts, with_events)]
    return bufs, evs


def _batch_fused(b, p, dt, lo, hi, meas, has, bufs, gate, policy):
    """the per-batch call on ticks [lo, hi): Batch.step_fused, or the C symbol for a batch that only predicts (meas_dev NULL)"""
    innov = None if bufs is None else (bufs[0], bufs[1])
    if meas is not None:
        b.step_fused(dt, meas[lo:hi], None if has is None else has[lo:hi], innov=innov, gate=gate, reacquire=policy)
        return
    ticks = hi - lo
    ins = None if innov is None else _innov_stream(innov, p["n"], p["m"], ticks)
    pol = None if policy is None else _reacquire(policy, p["n"], ticks)
    args = (None, 0, 0, None, 0, None, None if ins is None else C.byref(ins), 0.0 if gate is None else float(gate), None if pol is None else C.byref(pol))
    if np.ndim(dt) == 0:
        rc = b._lib.target_batch_step_fused_gated(b._h, ticks, float(dt), *args)
    else:
        sched = np.ascontiguousarray(dt, dtype=np.float64)
        rc = b._lib.target_batch_step_fused_dt(b._h, ticks, sched.ctypes.data_as(capi.c_double_p), *args)
    assert rc == 0, capi.last_error()


def _replay(mgr, parts, how, dt, calls, bufs, evs, gates, Ks, predict_only=(), masked=True):
    """the calls [(lo, hi), ...] on every batch: how = "all" (step_fused_all) or "per" (the per-batch calls in batch order).  Streams with
    as many blocks as the longest call are linear for it; shorter ones are rings."""
    bs = mgr.batches()
    for lo, hi in calls:
        meas = [None if p["name"] in predict_only else p["soa"] for p in parts]
        has = [p["has"] if masked and p["name"] not in predict_only else None for p in parts]
        pol = [None if K is None else (K, ev) for K, ev in zip(Ks, evs)]
        d = dt if np.ndim(dt) == 0 else list(dt[lo:hi])
        if how == "all":
            kw = {}
            if any(x is not None for x in bufs):
                kw["innov"] = bufs
            if any(g is not None for g in gates):
                kw["gate"] = gates
            if any(x is not None for x in pol):
                kw["reacquire"] = pol
            mgr.step_fused_all(d, [None if t is None else t[lo:hi] for t in meas], [None if h is None else h[lo:hi] for h in has], n_ticks=hi - lo, **kw)
        else:
            for b, p, t, h, bf, g, po in zip(bs, parts, meas, has, bufs, gates, pol):
                _batch_fused(b, p, d, lo, hi, t, h, bf, g, po)


def _collect(mgr, parts, bufs, evs, stride=1):
    """everything that can be read back, per part (counters and times of every stride-th target)"""
    out = []
    for b, p, bf, ev in zip(mgr.batches(), parts, bufs, evs):
        d = dict(runs=b.rejection_runs(), shared=b.shared_axes)
        d["x"], d["P"] = mgr.get_state_batch(p["ids"])
        some = p["ids"][::stride]
        d["nm"] = np.array([mgr.getNumberMeasurements(int(i)) for i in some])
        d["t"] = np.array([mgr.getTime(int(i)) for i in some])
        if bf is not None:
            d["nis"], d["nu"] = _read(bf, p["n"])
        if ev is not None:
            d["events"] = _read_events(ev, p["n"])
        out.append(d)
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.keys() == w.keys()
        for k in g:
            np.testing.assert_array_equal(g[k], w[k], err_msg="%s: batch %d: %s" % (what, i, k))


def _both(models, part_list, dtype, ticks, calls, dt=DT, innov=None, events=None, gates=None, Ks=None, blocks=None, predict_only=(), masked=True,
          served=None, gated=False, scheduled=False, after=None, stride=1, **mk):
    """two managers from the same inputs, one through step_fused_all, one through the per-batch calls: everything read back from both"""
    out = {}
    for how in ("all", "per"):
        nb = len(part_list)
        parts = [_part(n, k, dtype, ticks, nan_target=bool(g)) for (n, k), g in zip(part_list, gates or [None] * nb)]
        mgr = _manager(models, parts, dtype, **mk)
        if served is not None and how == "all":
            assert mgr.fused_all_served(gated=gated, scheduled=scheduled) == served
        bufs, evs = _streams(parts, blocks or ticks, innov or [False] * nb, events or [False] * nb)
        _replay(mgr, parts, how, dt, calls, bufs, evs, gates or [None] * nb, Ks or [None] * nb, predict_only, masked)
        if after is not None:
            after(mgr, parts)
        out[how] = _collect(mgr, parts, bufs, evs, stride)
        out[how + " parts"] = parts
        mgr.close()
    return out


# ---------------------------------------------------------------------------------------------------------- mixed populations
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("part_list", [FOUR, TWO], ids=["four models", "AR + UA"])
def test_plain_loop_equals_per_batch_calls(models, part_list, dtype):
    """7 ticks with a mask that misses some targets on some ticks, one batch predict-only: the plain loop, one launch."""
    out = _both(models, part_list, dtype, 7, [(0, 7)], predict_only=(UA,), served=1)
    _same(out["all"], out["per"], "plain %s" % dtype)
    assert all(np.isfinite(d["x"]).all() for d in out["all"])
    for d, p in zip(out["all"], out["all parts"]):
        want = np.zeros(p["n"], int) if p["name"] == UA else p["mask"].sum(0)
        np.testing.assert_array_equal(d["nm"], want)
        assert (d["t"] == d["t"][0]).all() and d["t"][0] > 0


def test_four_wavefronts_per_workgroup_grid(models):
    """UV fp32 with 66 000 targets (1032 wavefronts > 1024: four per workgroup) plus UA with 300, 3 ticks: the smallest population
    that takes that grid, with a ragged last workgroup in each part."""
    out = _both(models, [(UV, 66000), (UA, 300)], "f32", 3, [(0, 3)], served=1, stride=997)
    _same(out["all"], out["per"], "four wavefronts per workgroup")
    assert all(np.isfinite(d["x"]).all() for d in out["all"])


# ------------------------------------------------------------------------------------------------------------- gate and policy
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gated_loop_equals_per_batch_calls(models, dtype):
    """Outliers on every model and NaN measurements on every gated one, K = 0, 2 and none, one batch with nis_max = 0 (the plain stream), NIS and event
    rings shorter than the calls, two consecutive calls (the runs carry over), then one ordinary step_sequence_all tick."""
    gates = [gate_ref.CHI2_99[3], gate_ref.CHI2_99[6], 0.0, 300.0]   # UV, AR, UA (plain stream), AV
    Ks = [2, 0, None, None]                                          # UV re-acquires, AR counts, UA / AV: no policy (K = -1)

    def one_more_tick(mgr, parts):
        mgr.step_sequence_all(DT, [p["soa"][14:15] for p in parts], [p["has"][14:15] for p in parts], use_graph=False)
    out = _both(models, FOUR, dtype, 15, [(0, 7), (7, 14)], innov=[True] * 4, events=[True, True, False, False], gates=gates, Ks=Ks, blocks=5,
                served=1, gated=True, after=one_more_tick)
    _same(out["all"], out["per"], "gated %s" % dtype)
    assert all(np.isfinite(d["x"]).all() and np.isfinite(d["P"]).all() for d in out["all"]), "a rejected NaN measurement reached the state"
    uv, ar, ua, av = out["all"]
    parts = out["all parts"]
    assert ((uv["events"] & 0x80) != 0).any() or uv["runs"].any(), "the gate never bit on uniform_velocity"
    assert ar["runs"].max() >= 1, "K = 0 counted nothing on angular_rates"
    assert not ua["runs"].any() and not av["runs"].any()
    for d, p, g in zip(out["all"], parts, gates):
        last = d["nis"][6 % 5]   # the ring's row of the second call's last tick (tick 6 of that call, tick 13 of the stream)
        has = p["mask"][13].astype(bool)
        assert (last[~has] == -1.0).all()
        if 0 < g < 20 and p["n"] > 1:   # (the chi-square gates; the rows are those of the last five ticks)
            assert np.isnan(d["nis"]).any() or (d["nis"] > g).any(), "%s: nothing was rejected" % p["name"]


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_schedule(models, dtype, gated):
    """A jittered dt list with a 0.0 entry, plain and gated; then a call of one tick."""
    dts = DT * np.array([1.0, 0.7, 1.31, 0.0, 1.0, 2.5, 0.93, 1.0])
    kw = dict(innov=[True] * 4, events=[True, False, True, False], gates=[11.345, 16.812, 0.0, 300.0], Ks=[2, None, None, None]) if gated else {}
    out = _both(models, FOUR, dtype, 8, [(0, 7), (7, 8)], dt=dts, served=1, gated=gated, scheduled=True, **kw)
    _same(out["all"], out["per"], "schedule %s" % dtype)
    assert all((d["t"] == d["t"][0]).all() for d in out["all"])


# --------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_against_the_oracle(models, dtype):
    """The plain loop against the oracle stepped per model, within test_gpu_parity's TOL: the suite is not self-referential.  (The stream
    without its outliers: an ungated filter follows a 0.5 m outlier, which says nothing about the launch.)"""
    parts = [_part(n, k, dtype, 7, clean=True) for n, k in FOUR]
    mgr = _manager(models, parts, dtype)
    assert mgr.fused_all_served() == 1
    mgr.step_fused_all(DT, [p["soa"] for p in parts], [p["has"] for p in parts])
    for p in parts:
        mdl = models[p["name"]]
        orc = oracle.OracleBatch(mdl["model"], mdl["Q"], mdl["R"], mdl["P"], p["p0"], DT, 0.0, dtype=dtype)
        tdt = np.float32 if dtype == "f32" else np.float64
        for s in range(7):
            orc.step(DT, p["meas"][s].astype(tdt).astype(np.float64), p["mask"][s])
        ex, ep = check_state(mgr, p["ids"], orc, dtype, "%s %s step_fused_all" % (p["name"], dtype))
        print("%s %s: worst |dx| %.3g, worst |dP| / max|P| %.3g" % (p["name"], dtype, ex, ep))
    mgr.close()


# --------------------------------------------------------------------------------------------------------------------- routing
def test_fallback_one_batch(models):
    out = _both(models, [(AR, 65)], "f64", 7, [(0, 7)], served=0)
    _same(out["all"], out["per"], "one batch")


def test_fallback_two_classes(models):
    out = _both(models, TWO, "f64", 7, [(0, 7)], innov=[True, True], gates=[11.345, 16.812], served=0, gated=True, two_classes_in=UA)
    _same(out["all"], out["per"], "two (Q, R) classes")


def test_fallback_only_one_batch_has_a_stream(models):
    out = _both(models, TWO, "f32", 7, [(0, 7)], innov=[False, True], events=[False, True], gates=[None, 16.812], Ks=[None, 2], served=1)
    _same(out["all"], out["per"], "a stream on one batch only")


def test_fallback_poses(models):
    got = {}
    for how in ("all", "per"):
        parts = [_part(n, k, "f64", 7) for n, k in TWO]
        mgr = _manager(models, parts, "f64")
        poses = [torch.full((7, 7, p["ld"]), float("nan"), dtype=torch.float64, device="cuda") for p in parts]
        if how == "all":
            mgr.step_fused_all(DT, [p["soa"] for p in parts], [p["has"] for p in parts], poses=poses)
        else:
            for b, p, ps in zip(mgr.batches(), parts, poses):
                b.step_fused(DT, p["soa"], p["has"], poses=ps)
        got[how] = _collect(mgr, parts, [None, None], [None, None])
        for d, p, ps in zip(got[how], parts, poses):
            h = ps.cpu().numpy()
            assert np.isnan(h[:, :, p["n"]:]).all() and np.isfinite(h[:, :, :p["n"]]).all()
            d["poses"] = h[:, :, :p["n"]]
        mgr.close()
    _same(got["all"], got["per"], "a call with poses")


def test_fallback_keep_measurement(models):
    got = {}
    for how in ("all", "per"):
        parts = [_part(n, k, "f64", 7) for n, k in TWO]
        mgr = _manager(models, parts, "f64")
        assert mgr.fused_all_served() == 1
        mgr.set_keep_measurement(True)
        assert mgr.fused_all_served() == 0
        _replay(mgr, parts, how, DT, [(0, 7)], [None, None], [None, None], [None, None], [None, None])
        got[how] = _collect(mgr, parts, [None, None], [None, None])
        mgr.close()
    _same(got["all"], got["per"], "keep_measurement")


def test_default_fp64_manager_is_expanded_first(models):
    """A default fp64 manager keeps its batches in the shared-axes form: it reports what the plain form reports, the call expands
    every batch first (target_batch_shared_axes 0 afterwards) and the bits are the per-batch calls'."""
    out = _both(models, FOUR, "f64", 7, [(0, 7)], innov=[True] * 4, gates=[11.345, 16.812, 9.0, 300.0], served=1, gated=True, shared=True, lanes=0)
    assert all(d["shared"] == 0 for d in out["all"]) and all(d["shared"] == 0 for d in out["per"])
    _same(out["all"], out["per"], "shared axes")
    parts = [_part(n, k, "f64", 2) for n, k in TWO]
    mgr = _manager(models, parts, "f64", shared=True, lanes=0)
    assert [b.shared_axes for b in mgr.batches()] == [1, 1] and mgr.fused_all_served() == 1 and mgr.fused_all_served(scheduled=True) == 1
    mgr.close()


def test_two_shards_on_one_device(models):
    """Batches spread over two shards of one device: one launch per shard, specs shard-major -- the bits of the per-batch calls."""
    ids_of = {}
    got = {}
    for how in ("all", "per"):
        parts = [_part(n, k, "f64", 7) for n, k in FOUR]
        mgr = _manager_sharded(models, parts)
        order = _shard_major(mgr, parts)
        ids_of[how] = [tuple(p["ids"][:3]) for p in order]
        nb = len(order)
        bufs, evs = _streams(order, 7, [True] * nb, [False] * nb)
        _replay(mgr, order, how, DT, [(0, 7)], bufs, evs, [9.0] * nb, [None] * nb)
        got[how] = _collect(mgr, order, bufs, evs)
        mgr.close()
    assert ids_of["all"] == ids_of["per"]
    _same(got["all"], got["per"], "two shards")


def _manager_sharded(models, parts):
    mgr = te.TargetManager(dtype="f64", lanes_per_target=301, shared_axes=False, devices=[0, 0])
    base = 0
    for p in parts:
        mdl = models[p["name"]]
        p["ids"] = np.arange(p["n"], dtype=np.uint32) * 3 + 1 + base
        base += 3 * p["n"] + 7
        assert mgr.init_batch(p["ids"], DT, 0.0, p["p0"], type=mdl["model"], Q=mdl["Q"], R=mdl["R"], P0=mdl["P"]) == p["n"]
    return mgr


def _shard_major(mgr, parts):
    """one part per batch of mgr.batches() (shard-major), cut to the ids that batch holds"""
    order = []
    by_first = {}
    for p in parts:
        for j, i in enumerate(p["ids"]):
            by_first[int(i)] = (p, j)
    for b in mgr.batches():
        ids = b.slot_ids()
        p, _ = by_first[int(ids[0])]
        cols = np.array([by_first[int(i)][1] for i in ids])
        ld = len(ids) + 13
        q = dict(name=p["name"], n=len(ids), m=p["m"], ld=ld, ids=ids.astype(np.uint32), p0=p["p0"][cols], meas=p["meas"][:, cols], mask=p["mask"][:, cols])
        q["soa"] = _soa(q["meas"], "f64", ld)
        q["has"] = torch.from_numpy(np.ascontiguousarray(q["mask"])).cuda()
        order.append(q)
    return order


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_batch_unchanged(models):
    """Each refusal: a negative code with a reason, and every batch as it was -- state bits, runs, counters, times, buffers and the
    storage form (a default fp64 manager: a refused call must not expand anything)."""
    parts = [_part(n, k, "f64", 4) for n, k in TWO]
    mgr = _manager(models, parts, "f64", shared=True, lanes=0)
    bs = mgr.batches()
    nb = len(parts)
    bufs, evs = _streams(parts, 4, [True] * nb, [True] * nb)
    lib, h = mgr._lib, mgr._h
    before = _collect(mgr, parts, [None] * nb, [None] * nb)
    assert all(d["shared"] == 1 for d in before)

    keep = []   # (the arrays behind the pointers handed to the library)

    def specs(ld_of=None, ring=0, count=nb):
        s = (capi.BatchSequence * max(count, 1))()
        keep.append(s)
        for i, p in enumerate(parts[:count]):
            s[i].meas_dev, s[i].tick_stride, s[i].ld = p["soa"].data_ptr(), p["soa"].stride(0), p["soa"].stride(1) if ld_of is None else ld_of(p)
            s[i].has_meas_dev, s[i].has_stride, s[i].ring_ticks = p["has"].data_ptr(), p["has"].stride(0), ring
        return C.cast(s, C.c_void_p)
    iss = (capi.InnovStream * nb)()
    rqs = (capi.Reacquire * nb)()
    for i, p in enumerate(parts):
        iss[i] = _innov_stream(bufs[i], p["n"], p["m"], 4)
        rqs[i] = _reacquire((2, evs[i]), p["n"], 4)
    gates = (C.c_double * nb)(9.0, 9.0)
    no_gate = (C.c_double * nb)(9.0, 0.0)
    dts = (C.c_double * 4)(DT, DT, DT, DT)
    refusals = [
        ("a policy without a gate", lambda: lib.target_manager_step_fused_all(h, 4, DT, specs(), None, iss, no_gate, rqs, nb), "needs the gate"),
        ("ld < size", lambda: lib.target_manager_step_fused_all(h, 4, DT, specs(ld_of=lambda p: p["n"] - 1), None, iss, gates, rqs, nb), "ld"),
        ("ld < size, no streams", lambda: lib.target_manager_step_fused_all(h, 4, DT, specs(ld_of=lambda p: p["n"] - 1), None, None, None, None, nb), "ld"),
        ("ring_ticks != 0", lambda: lib.target_manager_step_fused_all(h, 4, DT, specs(ring=4), None, iss, gates, rqs, nb), "ring_ticks"),
        ("the wrong number of specs", lambda: lib.target_manager_step_fused_all(h, 4, DT, specs(count=1), None, iss, gates, rqs, 1), "one spec per batch"),
        ("dt_host NULL", lambda: lib.target_manager_step_fused_all_dt(h, 4, None, specs(), None, iss, gates, rqs, nb), "dt_host"),
    ]
    for what, refused, reason in refusals:
        rc = refused()
        err = capi.last_error()
        assert rc < 0 and reason in err, (what, rc, err)
        _same(_collect(mgr, parts, [None] * nb, [None] * nb), before, what)
        for bf, ev in zip(bufs, evs):
            assert (torch.isnan(bf[0]).all() and torch.isnan(bf[1]).all() and (ev == PAD).all()).item(), what + ": a refused call wrote rows"
    # ... and the same arguments, accepted
    assert lib.target_manager_step_fused_all_dt(h, 4, dts, specs(), None, iss, gates, rqs, nb) == 0, capi.last_error()
    assert [b.shared_axes for b in bs] == [0, 0]
    assert lib.target_manager_step_fused_all_served(None, 0, 0) == -1
    mgr.close()
