"""Step sequences and fused replays with a time step per tick (target_batch_step_sequence_dt, target_batch_step_fused_dt,
target_manager_step_sequence_all_dt; a sequence-valued dt in manager.py).  The contract: per slot, the call equals single ticks
with dt = schedule[s], bit for bit -- state, covariance, counters, rejection runs, every stream row, the target's time.

The stream is tests/reacquire_ref.py's: 203 targets (three full wavefronts and a ragged one of 11), 20 ticks, masked ticks,
outliers, the jump; ld = N + 13, the padding never written.  The schedule is tests/dt_schedule_ref.py's: DT * f[s], f seeded over
[0.25, 2], one tick at exactly 0.0 and one at 3 DT.  With the twin stepped at that schedule the chi-square 0.99 gate with K = 3
rejects 660 / 701 / 461 / 462 measurements and re-initialises 116 / 133 / 59 / 59 times (uniform_velocity, uniform_acceleration,
angular_rates, angular_velocities; tests/test_dt_schedule_reference.py holds the floor of 10 and 3), so the gated tests are not
vacuous."""
import ctypes as C
import functools

import numpy as np
import pytest

import dt_schedule_ref as ds
import gate_ref
import innov_stream_ref as ref
import reacquire_ref as rq
from conftest import HARNESS_ORDER
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from target_estimation_amd import capi  # noqa: E402
from test_gpu_gate import _counts  # noqa: E402
from test_gpu_innov_stream import _bufs, _init, _manager, _read, _soa  # noqa: E402
from test_gpu_reacquire import _events, _read_events  # noqa: E402

N, TICKS, DT = rq.N, rq.TICKS, rq.DT
LD = N + 13
IDS = np.arange(N, dtype=np.uint32) * 3 + 1
SCHED = ds.SCHEDULE
CASES = [(m, d, g) for m in HARNESS_ORDER for d in ("f64", "f32") for g in (201, 301)]
PLAIN_KEYS = ("x", "P", "nm", "t")
GATED_KEYS = PLAIN_KEYS + ("nis", "nu", "events", "runs")


@functools.lru_cache(maxsize=None)
def _tensors(name, dtype):
    p0, meas, mask, _, _ = rq.stream(name)
    return p0, meas, mask, _soa(meas, dtype, LD), torch.from_numpy(mask.copy()).cuda()


def _collect(mgr, b, ids, bufs=None, ev=None):
    out = {}
    if bufs is not None:
        out["nis"], out["nu"] = _read(bufs, len(ids))
        out["events"] = _read_events(ev, len(ids))
        out["runs"] = b.rejection_runs()
    out["x"], out["P"] = mgr.get_state_batch(ids)
    out["nm"] = _counts(mgr, ids)
    out["t"] = np.array([mgr.getTime(int(i)) for i in ids])
    return out


def _run(name, dtype, lanes, how, gated, sched=SCHED, splits=None, kw=None, shared=None, served=None):
    """one fresh manager over the stream.  how: "fused" / "sequence" / "graph" take the schedule in one call per split;
    "single" is the reference: one tick per call with the scalar dt = sched[s] (b.step, or with `gated` the gated single-tick
    sequence call)."""
    kw = kw or {}
    p0, meas, mask, soa, has = _tensors(name, dtype)
    mgr = _manager(name, dtype, lanes, **kw, **({} if shared is None else dict(shared_axes=shared)))
    _init(mgr, IDS, p0, **kw)
    b = mgr.batches()[0]
    if served is not None:
        assert b.fused_dt_served(gated) == served, (name, dtype, lanes, how)
    m = gate_ref.m_of(name)
    gamma = gate_ref.CHI2_99[m]
    ticks = len(sched)
    bufs, ev = (_bufs(ticks, m, LD), _events(ticks, LD)) if gated else (None, None)

    def streams(lo, hi):
        return dict(innov=(bufs[0][lo:hi], bufs[1][lo:hi]), gate=gamma, reacquire=(3, ev[lo:hi])) if gated else {}
    if how == "single":
        for s in range(ticks):
            if gated:
                b.step_sequence(float(sched[s]), soa[s:s + 1], has[s:s + 1], **streams(s, s + 1))
            else:
                b.step(float(sched[s]), soa[s], has[s])
    else:
        for lo, hi in splits or [(0, ticks)]:
            if how == "fused":
                b.step_fused(sched[lo:hi], soa[lo:hi], has[lo:hi], **streams(lo, hi))
            else:
                b.step_sequence(sched[lo:hi], soa[lo:hi], has[lo:hi], use_graph=(how == "graph"), **streams(lo, hi))
    out = _collect(mgr, b, IDS, bufs, ev)
    out["served"] = b.fused_dt_served(gated)
    out["recordings"] = b.graph_recordings
    mgr.close()
    return out


@functools.lru_cache(maxsize=None)
def _single(name, dtype, lanes, gated):
    return _run(name, dtype, lanes, "single", gated)


def _same(got, want, what, keys):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


@pytest.mark.parametrize("name,dtype,lanes", CASES)
def test_schedule_calls_equal_single_ticks(name, dtype, lanes):
    """1.  One step_fused(dt=schedule) call and one step_sequence(dt=schedule) call, eager and recorded, against a second manager
    calling b.step(dt[s], ...) tick by tick: x, P, counters and times bit for bit."""
    want = _single(name, dtype, lanes, False)
    assert len(set(want["t"])) == 1 and want["t"][0] > 0.0
    for how in ("fused", "sequence", "graph"):
        got = _run(name, dtype, lanes, how, False)
        _same(got, want, "%s %s %d %s" % (name, dtype, lanes, how), PLAIN_KEYS)
        if how == "fused":
            assert got["served"] == 1, "the plain fused loop with the table exists for every model on the separable layouts"


@pytest.mark.parametrize("name,dtype,lanes", CASES)
def test_gated_schedule_calls_equal_gated_single_ticks(name, dtype, lanes):
    """2.  The same with innov=, gate= (chi-square 0.99) and reacquire=(3, events): NIS, nu, events and runs as well.  One launch
    is required for the two linear models in both precisions; elsewhere 0 is allowed and the equality holds all the same.
    With the twin stepped at dt[s] the gate rejects 660 / 701 / 461 / 462 measurements and re-initialises 116 / 133 / 59 / 59 times
    (uniform_velocity, uniform_acceleration, angular_rates, angular_velocities); the run here must show at least 10 and 3."""
    want = _single(name, dtype, lanes, True)
    mask = rq.stream(name)[2].astype(bool)
    rejected = (mask & ~((want["nis"] >= 0) & (want["nis"] <= gate_ref.CHI2_99[gate_ref.m_of(name)]))).sum()
    reinit = ((want["events"] & 0x80) != 0).sum()
    print("%s %s %d: %d rejections, %d re-initialisations" % (name, dtype, lanes, rejected, reinit))
    assert rejected >= 10 and reinit >= 3
    for how in ("fused", "sequence", "graph"):
        got = _run(name, dtype, lanes, how, True)
        _same(got, want, "%s %s %d %s" % (name, dtype, lanes, how), GATED_KEYS)
        if how == "fused":
            assert got["served"] in (0, 1)
            if name.startswith("uniform"):
                assert got["served"] == 1, "%s %s must be served by one launch" % (name, dtype)


@pytest.mark.parametrize("name,dtype", [("angular_rates", "f64"), ("uniform_acceleration", "f32")])
def test_pose_stream(name, dtype):
    """3.  poses= in the schedule calls: every block equals get_est_dev after the single tick, bit for bit."""
    p0, meas, mask, soa, has = _tensors(name, dtype)
    mgr = _manager(name, dtype)
    _init(mgr, IDS, p0)
    b = mgr.batches()[0]
    want = np.zeros((TICKS, 7, N))
    for s in range(TICKS):
        b.step(float(SCHED[s]), soa[s], has[s])
        want[s] = b.get_est(twist=False, acc=False)[0].cpu().numpy().T
    mgr.close()
    for how in ("fused", "sequence"):
        mgr = _manager(name, dtype)
        _init(mgr, IDS, p0)
        b = mgr.batches()[0]
        poses = torch.full((TICKS, 7, LD), float("nan"), dtype=torch.float64, device="cuda")
        (b.step_fused if how == "fused" else b.step_sequence)(SCHED, soa, has, poses=poses)
        torch.cuda.synchronize()
        h = poses.cpu().numpy()
        assert np.isnan(h[:, :, N:]).all(), "a pose column beyond the batch size was written"
        np.testing.assert_array_equal(h[:, :, :N], want, err_msg="%s %s %s" % (name, dtype, how))
        mgr.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_against_the_oracle(name, dtype):
    """4.  The ungated schedule, 301 lanes, against the twin stepped with dt[s]: final x and P within TOL[dtype], the NIS stream
    within the innovation stream's bounds."""
    p0, meas, mask, soa, has = _tensors(name, dtype)
    m = gate_ref.m_of(name)
    want = ds.twin(name, None, 0)
    mgr = _manager(name, dtype, 301)
    _init(mgr, IDS, p0)
    b = mgr.batches()[0]
    bufs = _bufs(TICKS, m, LD)
    b.step_fused(SCHED, soa, has, innov=bufs)
    nis, nu = _read(bufs, N)
    x, P = mgr.get_state_batch(IDS)
    mgr.close()
    what = "%s %s schedule" % (name, dtype)
    ref.check(nu, nis, want, mask, dtype, what)
    t = TOL[dtype]
    ex = np.abs(x - want["x"]).max()
    ep = max(np.abs(P[j] - want["P"][j]).max() / np.abs(want["P"][j]).max() for j in range(N))
    print("%s: worst |dx| %.3g, worst |dP| / max|P| %.3g" % (what, ex, ep))
    np.testing.assert_allclose(x, want["x"], atol=t["x_atol"], rtol=t["x_rtol"])
    for j in range(N):
        assert np.abs(P[j] - want["P"][j]).max() <= t["P_rel"] * np.abs(want["P"][j]).max()


@pytest.mark.parametrize("gated", [False, True])
def test_two_calls_without_a_synchronisation(gated):
    """5 (a).  Two fused schedule calls (ticks 0-9 and 10-19, different halves of the schedule) enqueued back to back equal one
    call: neither sees the other's table."""
    name, dtype = "uniform_acceleration", "f64"
    one = _run(name, dtype, 301, "fused", gated)
    assert one["served"] == 1
    two = _run(name, dtype, 301, "fused", gated, splits=[(0, 10), (10, 20)])
    _same(two, one, "two fused schedule calls", GATED_KEYS if gated else PLAIN_KEYS)
    _same(one, _single(name, dtype, 301, gated), "one fused schedule call", GATED_KEYS if gated else PLAIN_KEYS)


def test_a_long_schedule():
    """5 (b).  5 targets, 600 ticks in one call -- longer than any small fixed staging: the sequence over a 20-tick ring, the fused
    call over a [600, 7, ld] tensor; both equal single ticks."""
    name, dtype, n, ticks = "uniform_velocity", "f64", 5, 600
    p0, meas, mask, _, _ = rq.stream(name)
    ids = IDS[:n]
    soa = _soa(meas[:, :n], dtype, n + 3)
    has = torch.from_numpy(mask[:, :n].copy()).cuda()
    sched = DT * np.random.default_rng(5).uniform(0.25, 2.0, ticks)
    sched[7] = 0.0
    idx = torch.arange(ticks, device="cuda") % TICKS
    long_soa, long_has = soa[idx].contiguous(), has[idx].contiguous()
    out = {}
    for how in ("single", "sequence", "graph", "fused"):
        mgr = _manager(name, dtype)
        _init(mgr, ids, p0[:n])
        b = mgr.batches()[0]
        if how == "single":
            for s in range(ticks):
                b.step(float(sched[s]), soa[s % TICKS], has[s % TICKS])
        elif how == "fused":
            b.step_fused(sched, long_soa, long_has)
            assert b.fused_dt_served(False) == 1
        else:
            b.step_sequence(sched, soa, has, n_ticks=ticks, use_graph=(how == "graph"))
        out[how] = _collect(mgr, b, ids)
        mgr.close()
    for how in ("sequence", "graph", "fused"):
        _same(out[how], out["single"], "600 ticks, %s" % how, PLAIN_KEYS)


@pytest.mark.parametrize("ticks", [1, 2])
def test_short_calls(ticks):
    """5 (c).  A 1-tick call and a 2-tick call."""
    name, dtype = "angular_velocities", "f64"
    want = _run(name, dtype, 301, "single", True, sched=SCHED[:ticks])
    for how in ("fused", "sequence", "graph"):
        _same(_run(name, dtype, 301, how, True, sched=SCHED[:ticks]), want, "%d tick(s), %s" % (ticks, how), GATED_KEYS)
        _same(_run(name, dtype, 301, how, False, sched=SCHED[:ticks]), _run(name, dtype, 301, "single", False, sched=SCHED[:ticks]),
              "%d tick(s), %s, plain" % (ticks, how), PLAIN_KEYS)


def test_graph_reuse():
    """6.  The same schedule twice replays one recording; a changed entry records anew and gives the changed result (a stale graph
    would give the old one); 0.0 and -0.0 are different schedules."""
    name, dtype = "uniform_velocity", "f64"
    p0, meas, mask, soa, has = _tensors(name, dtype)
    half = TICKS // 2
    a = SCHED[:half].copy()
    c = a.copy()
    c[3] *= 1.5

    def run(first, second, use_graph):
        mgr = _manager(name, dtype)
        _init(mgr, IDS, p0)
        b = mgr.batches()[0]
        # (the same measurement block both times: a recording is filed under its buffers too)
        b.step_sequence(first, soa[:half], has[:half], use_graph=use_graph)
        r1 = b.graph_recordings
        b.step_sequence(second, soa[:half], has[:half], use_graph=use_graph)
        out = _collect(mgr, b, IDS)
        out["rec"] = (r1, b.graph_recordings)
        mgr.close()
        return out
    same, eager = run(a, a.copy(), True), run(a, a, False)
    assert same["rec"] == (1, 1), "the same schedule (another array, the same values) must replay the one recording"
    _same(same, eager, "the same schedule twice", PLAIN_KEYS)
    changed, eager_changed = run(a, c, True), run(a, c, False)
    assert changed["rec"] == (1, 2), "a changed entry must record anew"
    _same(changed, eager_changed, "a changed entry", PLAIN_KEYS)
    assert not np.array_equal(changed["x"], same["x"])
    z, nz = a.copy(), a.copy()
    z[2], nz[2] = 0.0, -0.0
    assert run(z, nz, True)["rec"] == (1, 2), "0.0 and -0.0 are compared as bits"
    # a scalar recording never serves a schedule of equal entries, nor the reverse
    assert run(DT, np.full(half, DT), True)["rec"] == (1, 2)


def _mixed(devices, n=130):
    from test_gpu_shards import _mixed as mixed
    return mixed(devices, n_uv=n, n_ua=n)


@pytest.mark.parametrize("use_graph", [False, True])
def test_manager_level(use_graph):
    """7.  Two models in one manager (one launch per tick for both), 130 targets each, 6 ticks, the query on:
    step_sequence_all(dt=schedule) equals per-batch single ticks plus the query; with devices=[0, 0, 0] it equals the one-shard
    manager bit for bit."""
    from test_gpu_shards import _batch_meas
    ticks = 6
    sched = SCHED[3:3 + ticks]          # (with the 0.0 tick)
    origin, radius = [0.3, -0.2, 0.1], 2.0
    res = {}
    for what, devices in (("single", None), ("all", None), ("sharded", [0, 0, 0])):
        mgr, ids = _mixed(devices)
        if devices is None:
            assert mgr.population_tick() == 1
        meas = _batch_meas(torch, mgr, ticks, 21)
        bs = mgr.batches()
        if what == "single":
            for s in range(ticks):
                for b, t in zip(bs, meas):
                    b.step(float(sched[s]), t[s])
            q = [b.intersect_sphere(origin, radius) for b in bs]
            deltas, qposes = [d for d, _ in q], [p for _, p in q]
        else:
            deltas = [torch.full((b.size,), float("nan"), dtype=torch.float64, device="cuda") for b in bs]
            qposes = [torch.full((b.size, 7), float("nan"), dtype=torch.float64, device="cuda") for b in bs]
            mgr.step_sequence_all(sched, meas, query=(origin, radius, deltas, qposes), use_graph=use_graph)
        mgr.synchronize()
        out = {}
        state = {}                      # (get_state_batch takes the ids of ONE model: batch by batch, then in id order)
        for b in bs:
            bid = b.slot_ids()
            xb, Pb = mgr.get_state_batch(bid)
            for j, i in enumerate(bid):
                state[int(i)] = (xb[j], Pb[j])
        out["x"] = np.concatenate([state[int(i)][0] for i in ids])
        out["P"] = np.concatenate([state[int(i)][1].ravel() for i in ids])
        out["nm"] = _counts(mgr, ids)
        out["t"] = np.array([mgr.getTime(int(i)) for i in ids])
        row = {int(i): k for k, i in enumerate(ids)}
        out["delta"], out["qpose"] = np.zeros(len(ids)), np.zeros((len(ids), 7))
        for b, d, p in zip(bs, deltas, qposes):
            rows = [row[int(i)] for i in b.slot_ids()]
            out["delta"][rows], out["qpose"][rows] = d.cpu().numpy(), p.cpu().numpy()
        res[what] = out
        mgr.close()
    keys = PLAIN_KEYS + ("delta", "qpose")
    _same(res["all"], res["single"], "step_sequence_all(dt=schedule) / single ticks", keys)
    _same(res["sharded"], res["all"], "three shards / one", keys)


def test_other_forms(models):
    """8.  A per-class batch, a coupled-Q (dense) batch and a shared-axes batch report served == 0 (the last: its call is the
    expansion and then the plain form's launch) and give equal results.  An all-equal schedule equals the scalar call: the bits of state and streams, the
    time within 1 ulp."""
    name, dtype = "uniform_velocity", "f64"
    mdl = models[name]
    Q, R, P0 = (np.asarray(mdl[k], float) for k in ("Q", "R", "P"))
    Qc = Q.copy()
    Qc[0, 1] = Qc[1, 0] = 0.1 * np.sqrt(Q[0, 0] * Q[1, 1])   # couples x and y: the dense kernels
    class_of = (np.arange(N) % 2).astype(np.uint32)
    routes = {
        "classes": (dict(kw=dict(classes=(np.stack([Q, 2.0 * Q]), np.stack([R, 1.5 * R]), np.stack([P0, P0]), class_of, mdl["model"]))), 0, 0),
        "coupled Q": (dict(kw=dict(QRP=(Qc, R, P0, mdl["model"]))), 0, 0),
        "shared axes": (dict(shared=True), 301, 0),
    }
    for what, (kw, lanes, served) in routes.items():
        for gated in (False, True):
            want = _run(name, dtype, lanes, "single", gated, **kw)
            for how in ("fused", "sequence"):
                got = _run(name, dtype, lanes, how, gated, served=served, **kw)
                _same(got, want, "%s %s gated %d" % (what, how, gated), GATED_KEYS if gated else PLAIN_KEYS)
    p0, meas, mask, soa, has = _tensors(name, dtype)
    m = gate_ref.m_of(name)
    for how in ("fused", "sequence"):
        out = {}
        for form in ("scalar", "schedule"):
            mgr = _manager(name, dtype)
            _init(mgr, IDS, p0)
            b = mgr.batches()[0]
            bufs, ev = _bufs(TICKS, m, LD), _events(TICKS, LD)
            (b.step_fused if how == "fused" else b.step_sequence)(DT if form == "scalar" else np.full(TICKS, DT), soa, has, innov=bufs,
                                                                   gate=gate_ref.CHI2_99[m], reacquire=(3, ev))
            out[form] = _collect(mgr, b, IDS, bufs, ev)
            mgr.close()
        _same(out["schedule"], out["scalar"], "an all-equal schedule, %s" % how, ("x", "P", "nm", "nis", "nu", "events", "runs"))
        ulp = np.spacing(np.abs(out["scalar"]["t"]))
        assert (np.abs(out["schedule"]["t"] - out["scalar"]["t"]) <= ulp).all()


def test_refusals():
    """9.  A NULL schedule and a sample of the scalar calls' refusals through the new symbols: a negative code with the reason,
    state untouched."""
    name, dtype = "uniform_velocity", "f64"
    m = gate_ref.m_of(name)
    p0, meas, mask, soa, has = _tensors(name, dtype)
    mgr = _manager(name, dtype)
    _init(mgr, IDS, p0)
    b = mgr.batches()[0]
    b.step_fused(SCHED[:2], soa[:2], has[:2])
    lib, h = b._lib, b._h
    before = (mgr.get_state_batch(IDS), _counts(mgr, IDS), mgr.getTime(int(IDS[0])), b.rejection_runs().copy())
    bufs, ev = _bufs(2, m, LD), _events(2, LD)
    sched = np.ascontiguousarray(SCHED[:2])
    dtp = sched.ctypes.data_as(capi.c_double_p)

    def stream(ptr=bufs[0].data_ptr(), ld=LD, stride=LD):
        s = capi.InnovStream()
        s.nis_dev, s.innov_dev, s.ld, s.nis_tick_stride, s.innov_tick_stride = ptr, bufs[1].data_ptr(), ld, stride, m * LD
        return s

    def policy(k=3):
        r = capi.Reacquire()
        r.max_rejects, r.event_dev, r.ld, r.tick_stride = k, ev.data_ptr(), LD, LD
        return r

    def fused(dt=dtp, nis_max=9.0, s=None, r=None, n_ticks=2, tick_stride=soa.stride(0), ld=soa.stride(1)):
        return lib.target_batch_step_fused_dt(h, n_ticks, dt, soa.data_ptr(), tick_stride, ld, has.data_ptr(), has.stride(0), None,
                                              None if s is None else C.byref(s), nis_max, None if r is None else C.byref(r))

    def seq(dt=dtp, nis_max=9.0, s=None, r=None, ring=0, use_graph=0):
        return lib.target_batch_step_sequence_dt(h, 2, dt, soa.data_ptr(), soa.stride(0), soa.stride(1), has.data_ptr(), has.stride(0), ring, None,
                                                 None if s is None else C.byref(s), nis_max, None if r is None else C.byref(r), use_graph)
    specs = (capi.BatchSequence * 2)()
    for spec in specs:
        spec.meas_dev, spec.tick_stride, spec.ld = soa.data_ptr(), soa.stride(0), soa.stride(1)

    def all_(dt=dtp, nb=1, query=0):
        return lib.target_manager_step_sequence_all_dt(mgr.handle, 2, dt, C.cast(specs, C.c_void_p), None, None, None, None, nb, query,
                                                       None, 1.0, 0)
    refusals = [
        ("fused: a NULL schedule", lambda: fused(dt=None, nis_max=0.0), "dt_host"),
        ("sequence: a NULL schedule", lambda: seq(dt=None, nis_max=0.0), "dt_host"),
        ("sequence, recorded: a NULL schedule", lambda: seq(dt=None, nis_max=0.0, use_graph=1), "dt_host"),
        ("all batches: a NULL schedule", lambda: all_(dt=None), "dt_host"),
        ("fused: a policy without a gate", lambda: fused(nis_max=0.0, s=stream(), r=policy()), "needs the gate"),
        ("fused: a gate without a stream", lambda: fused(), "nis_dev"),
        ("fused: max_rejects > 127", lambda: fused(s=stream(), r=policy(k=128)), "max_rejects"),
        ("fused: NIS rows with ld < size", lambda: fused(s=stream(ld=N - 1, stride=N - 1)), "ld"),
        ("fused: n_ticks beyond an int", lambda: fused(s=stream(), n_ticks=1 << 31), ""),
        ("fused: a negative tick_stride", lambda: fused(s=stream(), tick_stride=-soa.stride(0)), "stride"),
        ("fused: measurements with ld < size", lambda: fused(s=stream(), ld=N - 1), "ld"),
        ("sequence: a gate without a stream", lambda: seq(), "nis_dev"),
        ("sequence: a negative ring", lambda: seq(nis_max=0.0, ring=-1), "ring_ticks"),
        ("sequence: nis_max NaN", lambda: seq(nis_max=float("nan"), s=stream()), "nis_max"),
        ("all batches: the wrong number of batches", lambda: all_(nb=2), "spec"),
        ("all batches: a query without an origin", lambda: all_(query=1), "query"),
    ]
    for what, refused, reason in refusals:
        rc = refused()
        err = lib.target_manager_last_error().decode()
        assert rc < 0 and reason in err, (what, rc, err)
        x, P = mgr.get_state_batch(IDS)
        np.testing.assert_array_equal(x, before[0][0], err_msg=what)
        np.testing.assert_array_equal(P, before[0][1], err_msg=what)
        np.testing.assert_array_equal(_counts(mgr, IDS), before[1], err_msg=what)
        assert mgr.getTime(int(IDS[0])) == before[2], what
        np.testing.assert_array_equal(b.rejection_runs(), before[3], err_msg=what)
        assert (torch.isnan(bufs[0]).all() and torch.isnan(bufs[1]).all()).item(), what + ": a refused call wrote rows"
    assert lib.target_batch_step_fused_dt_served(None, 0) == -1
    assert fused(dt=None, nis_max=0.0, n_ticks=0) == 0, "no ticks need no schedule"
    with pytest.raises(ValueError):
        b.step_fused(SCHED[:3], soa[:2], has[:2])
    mgr.close()
