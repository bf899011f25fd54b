"""The NIS gate and the re-acquisition policy INSIDE resident sessions (target_batch_live_set_gate): a gated session decides
between prediction and update, keeps the rejection runs and re-initialises lost targets inside the resident kernel, tick after
tick, and writes per-tick NIS and event rows a consumer can read while the session runs.  Per slot and tick it must equal the
launched calls (step_sequence(..., innov=, gate=, reacquire=)) bit for bit.

The stream is tests/reacquire_ref.py's throughout: 203 targets (three full wavefronts and a ragged one of 11), 20 ticks, masked
ticks, +0.5 m outliers, yaw spikes on ticks 6 and 7, the jump at tick 8.  Every session runs with max_ticks = the ticks it posts
and an idle limit of 3 s, and waits only through live_wait with an asserted timeout: a failing test leaves no kernel behind."""
import functools

import numpy as np
import pytest

import gate_ref
import innov_stream_ref as ref
import oracle
import reacquire_ref as rq
from conftest import HARNESS_ORDER, model_path
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from test_gpu_gate import _accepted, _counts  # noqa: E402
from test_gpu_innov_stream import _init, _manager, _soa  # noqa: E402
from test_gpu_reacquire import PAD, _as_read, _feature, _host_rule  # noqa: E402

N, TICKS, DT = rq.N, rq.TICKS, rq.DT
LD = N + 13
IDS = np.arange(N, dtype=np.uint32) * 3 + 1
CASES = [(m, d) for m in HARNESS_ORDER for d in ("f64", "f32")]
# every (model, precision) with resident kernels has a gated one; the two linear models in both precisions and the angular
# models in fp64 MUST have (a batch that reports 0 there fails the tests below instead of passing by refusal)
MUST_SERVE = [(m, d) for m, d in CASES if not (m.startswith("angular") and d == "f32")]


def _rows(blocks):
    return (torch.full((blocks, LD), float("nan"), dtype=torch.float64, device="cuda"), torch.full((blocks, LD), PAD, dtype=torch.uint8, device="cuda"))


def _read_rows(nis, ev):
    torch.cuda.synchronize()
    a, e = nis.cpu().numpy(), ev.cpu().numpy()
    assert np.isnan(a[:, N:]).all(), "a NIS column beyond the batch size was written"
    assert (e[:, N:] == PAD).all(), "an event column beyond the batch size was written"
    return a[:, :N], e[:, :N]


def _tensors(name, dtype, meas=None, mask=None):
    p0, meas0, mask0, _, _ = rq.stream(name)
    meas, mask = meas0 if meas is None else meas, mask0 if mask is None else mask
    return p0, meas, mask, _soa(meas, dtype, LD), torch.from_numpy(mask.copy()).cuda()


def _live_manager(name, dtype, p0, ids=IDS):
    """a manager on a non-blocking stream of its own (work queued behind a resident kernel's stream would wait for the session)"""
    stream = torch.cuda.Stream()
    mgr = _manager(name, dtype)
    mgr.set_stream(stream.cuda_stream)
    _init(mgr, ids, p0)
    mgr.synchronize()
    return mgr, mgr.batches()[0], stream


def _refused_instead(b, name, dtype, nis):
    """True if the batch has no gated resident kernel: the refusal is asserted in place of the case (never for MUST_SERVE)."""
    if b.live_gate_served == 1:
        return False
    assert (name, dtype) not in MUST_SERVE, "%s %s must have a gated resident kernel" % (name, dtype)
    with pytest.raises(RuntimeError, match="no gated resident kernel"):
        b.live_set_gate(1.0, nis)
    return True


def _ring_session(b, soa, has, ring, first=0):
    """ticks first.. of soa / has through a measurement ring of `ring` that the host refills on a second stream: one doorbell, then a
    doorbell per tick, then whole refills posted at once"""
    ticks = soa.shape[0] - first
    ring_m, ring_h = soa[first:first + ring].clone(), has[first:first + ring].clone()
    torch.cuda.synchronize()
    copy = torch.cuda.Stream()
    b.live_start(DT, ring_m, ring_h, max_ticks=ticks, idle_limit_s=3.0)
    try:
        b.live_post(1)
        assert b.live_wait(1, 5.0) and b.live_done() >= 1
        b.live_post_each(ring - 1)
        assert b.live_wait(ring, 5.0)
        done = ring
        while done < ticks:
            k = min(ring, ticks - done)
            with torch.cuda.stream(copy):
                ring_m[:k].copy_(soa[first + done:first + done + k])
                ring_h[:k].copy_(has[first + done:first + done + k])
            copy.synchronize()
            b.live_post(k)
            done += k
            assert b.live_wait(done, 5.0)
    finally:
        served = b.live_stop()
    assert served == ticks


def _state(mgr, b, ids=IDS):
    out = dict(runs=b.rejection_runs())
    out["x"], out["P"] = mgr.get_state_batch(ids)
    out["nm"] = _counts(mgr, ids)
    out["t"] = np.array([mgr.getTime(int(i)) for i in ids])
    return out


def _live_feature(name, dtype, gamma, K, meas=None, mask=None):
    """the stream through ONE gated session over a measurement ring of 8, NIS and event rows for every tick: the dict of _feature
    (without nu), or None where the batch has no gated kernel (the refusal asserted)"""
    p0, meas, mask, soa, has = _tensors(name, dtype, meas, mask)
    mgr, b, _stream = _live_manager(name, dtype, p0)
    nis, ev = _rows(TICKS)
    if _refused_instead(b, name, dtype, nis):
        mgr.close()
        return None
    ungated = b.live_capacity
    b.live_set_gate(gamma, nis, reacquire=None if K is None else (K, ev))
    assert N <= b.live_capacity <= ungated
    _ring_session(b, soa, has, 8)
    out = _state(mgr, b)
    out["nis"], out["events"] = _read_rows(nis, ev)
    mgr.close()
    return out


@functools.lru_cache(maxsize=None)
def _launched(name, dtype, gamma, K):
    """the reference: a second manager stepping the same stream with step_sequence(..., innov=, gate=, reacquire=(K, ev)), one tick per call"""
    p0, meas, mask, soa, has = _tensors(name, dtype)
    return _feature(name, dtype, 0, p0, soa, has, IDS, gate_ref.m_of(name), LD, gamma, K, splits=[(s, s + 1) for s in range(TICKS)])


def _same(got, want, what, keys=("x", "P", "nis", "events", "runs", "nm", "t")):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


@pytest.mark.parametrize("name,dtype", CASES)
def test_gated_session_equals_gated_single_ticks_bit_for_bit(name, dtype):
    """1.  The chi-square 0.99 gate with K = 3, the 20 ticks through a session over a ring of 8 refilled on a second stream, against
    a second manager stepping one tick per call with innov=, gate=, reacquire=(3, ev): x and P by id, NIS rows, event rows,
    rejection_runs(), measurement counters, times; padding untouched; at least 40 re-initialisations; angular models: some
    re-initialised target is measured on a later tick (the tail's record and its unwrap memory are then in use)."""
    m = gate_ref.m_of(name)
    gamma = gate_ref.CHI2_99[m]
    got = _live_feature(name, dtype, gamma, 3)
    if got is None:
        return
    want = _launched(name, dtype, gamma, 3)
    init = (got["events"] & 0x80) != 0
    print("%s %s: %d re-initialisations in the session" % (name, dtype, init.sum()))
    _same(got, want, "%s %s session / single ticks" % (name, dtype))
    assert init.sum() >= 40
    mask = rq.stream(name)[2]
    if m == 6:
        assert [(s, j) for s, j in zip(*np.nonzero(init)) if mask[s + 1:, j].any()], "no re-initialised target is measured on a later tick"
    np.testing.assert_array_equal(got["nm"], _accepted(got["nis"], mask, gamma).sum(0))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_against_the_twin(name, dtype):
    """2.  gamma = 300, K = 3: events and runs are the twin's exactly, no pair left out; NIS within the innovation stream's bounds;
    the final x, P within TOL[dtype]."""
    got = _live_feature(name, dtype, 300.0, 3)
    if got is None:
        return
    want = rq.reference(name, 300.0, 3)
    mask = rq.stream(name)[2]
    what = "%s %s gated session" % (name, dtype)
    np.testing.assert_array_equal(got["events"], want["event"], err_msg=what + ": an event differs from the twin's")
    np.testing.assert_array_equal(got["runs"], want["run"], err_msg=what)
    ref.check(None, got["nis"], want, mask, dtype, what)
    np.testing.assert_array_equal(got["nm"], want["acc"].sum(0))
    t = TOL[dtype]
    ex = np.abs(got["x"] - want["x"]).max()
    ep = max(np.abs(got["P"][j] - want["P"][j]).max() / np.abs(want["P"][j]).max() for j in range(N))
    print("%s: worst |dx| %.3g, worst |dP| / max|P| %.3g" % (what, ex, ep))
    np.testing.assert_allclose(got["x"], want["x"], atol=t["x_atol"], rtol=t["x_rtol"])
    for j in range(N):
        assert np.abs(got["P"][j] - want["P"][j]).max() <= t["P_rel"] * np.abs(want["P"][j]).max()


@pytest.mark.parametrize("name,dtype", [("uniform_acceleration", "f64"), ("angular_velocities", "f64")])
def test_rows_are_readable_while_the_session_runs(name, dtype):
    """3.  One tick posted at a time; after live_wait(k + 1) a copy on another stream of NIS row k % ring and event row k % ring
    equals the single-tick reference's row k -- for every k, the session still open."""
    m = gate_ref.m_of(name)
    gamma, ring = gate_ref.CHI2_99[m], 3
    want = _launched(name, dtype, gamma, 3)
    p0, meas, mask, soa, has = _tensors(name, dtype)
    mgr, b, _stream = _live_manager(name, dtype, p0)
    nis, ev = _rows(ring)
    b.live_set_gate(gamma, nis, reacquire=(3, ev))
    h_nis = torch.empty((LD,), dtype=torch.float64).pin_memory()
    h_ev = torch.empty((LD,), dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    copy = torch.cuda.Stream()
    b.live_start(DT, soa, has, max_ticks=TICKS, idle_limit_s=3.0)
    try:
        for k in range(TICKS):
            b.live_post(1)
            assert b.live_wait(k + 1, 5.0)
            with torch.cuda.stream(copy):
                h_nis.copy_(nis[k % ring], non_blocking=True)
                h_ev.copy_(ev[k % ring], non_blocking=True)
            copy.synchronize()
            assert b.live_running()
            np.testing.assert_array_equal(h_nis.numpy()[:N], want["nis"][k], err_msg="NIS row of tick %d, read mid-session" % k)
            np.testing.assert_array_equal(h_ev.numpy()[:N], want["events"][k], err_msg="event row of tick %d, read mid-session" % k)
    finally:
        served = b.live_stop()
    assert served == TICKS
    _same(_state(mgr, b), want, "%s %s one tick at a time" % (name, dtype), keys=("x", "P", "runs", "nm", "t"))
    mgr.close()


@pytest.mark.parametrize("name,dtype", [("uniform_velocity", "f32"), ("angular_rates", "f64")])
def test_gate_only_and_k0(name, dtype):
    """4.  K = 0: the runs count and nothing is re-initialised, every output bit-equal to the launched call.  Gate only (reacquire=None)
    behind it on the same batch: the runs read after the session are the bytes from before it, state and NIS those of the launched
    gate= call on a manager with the same history."""
    m, gamma = gate_ref.m_of(name), 300.0
    got = _live_feature(name, dtype, gamma, 0)
    want = _launched(name, dtype, gamma, 0)
    _same(got, want, "%s %s K = 0" % (name, dtype))
    assert not (got["events"] & 0x80).any() and got["runs"].max() >= 4
    # gate only: ticks 0-9 with K = 0 by the launched call on both managers (the runs are then not all zero), ticks 10-19 gate only
    p0, meas, mask, soa, has = _tensors(name, dtype)
    half = TICKS // 2
    out = {}
    for how in ("session", "launched"):
        mgr, b, _stream = _live_manager(name, dtype, p0)
        nis, ev = _rows(TICKS)
        b.step_sequence(DT, soa[:half], has[:half], innov=(nis[:half], None), gate=gamma, reacquire=(0, ev[:half]))
        before = b.rejection_runs().copy()
        assert before.any()
        if how == "session":
            b.live_set_gate(gamma, nis[half:])
            _ring_session(b, soa, has, 5, first=half)
        else:
            for s in range(half, TICKS):
                b.step_sequence(DT, soa[s:s + 1], has[s:s + 1], innov=(nis[s:s + 1], None), gate=gamma)
        out[how] = _state(mgr, b)
        np.testing.assert_array_equal(out[how]["runs"], before, err_msg="a gate without a policy touched the rejection runs (%s)" % how)
        out[how]["nis"], events = _read_rows(nis, ev)
        assert (events[half:] == PAD).all(), "a gate without a policy wrote event rows"
        mgr.close()
    _same(out["session"], out["launched"], "%s %s gate only" % (name, dtype), keys=("x", "P", "nis", "runs", "nm", "t"))


@pytest.mark.parametrize("name,dtype", [("uniform_acceleration", "f32"), ("angular_rates", "f64"), ("angular_velocities", "f64")])
def test_nan_and_zero_quaternion_measurements(name, dtype):
    """5.  Target A gets NaN on ticks 5-7 and the +0.5 m jump from tick 8; angular models: target B gets the jump and a zero quaternion
    on ticks 8-10.  They reject and never re-initialise while degenerate, exactly as in the launched call; no NaN reaches x or P."""
    m, gamma = gate_ref.m_of(name), 300.0
    p0, meas, mask, outlier, spikes = gate_ref.stream(name)
    meas, mask = meas.copy(), mask.copy()
    busy = {j for _, j in spikes}
    free = [j for j in range(N) if not outlier[:, j].any() and j not in busy]
    A, B = free[0], free[1]
    mask[2:11, [A, B]] = 1
    meas[5:8, A, 0] = np.nan
    meas[8:, A, 0] += rq.JUMP
    if m == 6:
        meas[8:, B, 0] += rq.JUMP
        meas[8:11, B, 3:7] = 0.0
    got = _live_feature(name, dtype, gamma, 3, meas, mask)
    p0, _, _, soa, has = _tensors(name, dtype, meas, mask)
    want = _feature(name, dtype, 0, p0, soa, has, IDS, m, LD, gamma, 3)
    _same(got, want, "%s %s NaN / zero quaternion" % (name, dtype))
    ev = got["events"]
    np.testing.assert_array_equal(ev[5:9, A], [1, 2, 3, 0x84])
    assert np.isnan(got["nis"][5:8, A]).all()
    if m == 6:
        np.testing.assert_array_equal(ev[8:11, B], [1, 2, 3])
        later = [s for s in range(11, TICKS) if mask[s, B]]
        assert later and ev[later[0], B] == 0x84
    assert np.isfinite(got["x"]).all() and np.isfinite(got["P"]).all()
    mdl = oracle.load_model_yaml(model_path(name))["model"]
    want_ev, want_run = _host_rule(mdl, got["nis"], mask, _as_read(meas, dtype), gamma, 3)
    np.testing.assert_array_equal(ev, want_ev)
    np.testing.assert_array_equal(got["runs"], want_run)


@pytest.mark.parametrize("name,dtype", [("uniform_velocity", "f64"), ("angular_velocities", "f64")])
def test_with_the_pose_output_and_the_per_tick_query(name, dtype):
    """6.  The pose output and the per-tick query in the same gated session: the poses of every tick equal get_est after the
    reference's same tick -- for the re-initialised targets too -- and the query's delta and pose the launched fused query's."""
    m = gate_ref.m_of(name)
    gamma = gate_ref.CHI2_99[m]
    p0, meas, mask, soa, has = _tensors(name, dtype)
    origin, radius = np.zeros(3), 5.0
    ref_mgr = _manager(name, dtype)
    _init(ref_mgr, IDS, p0)
    rnis, rev = _rows(TICKS)
    rd, rp = torch.zeros((N,), dtype=torch.float64, device="cuda"), torch.zeros((N, 7), dtype=torch.float64, device="cuda")
    want = []
    for s in range(TICKS):
        ref_mgr.step_sequence_all(DT, [soa[s:s + 1]], [has[s:s + 1]], query=(origin, radius, [rd], [rp]), use_graph=0,
                                  innov=[(rnis[s:s + 1], None)], gate=gamma, reacquire=(3, rev[s:s + 1]))
        torch.cuda.synchronize()
        want.append((ref_mgr.batches()[0].get_est(twist=False, acc=False)[0].cpu().numpy().copy(), rd.cpu().numpy().copy(), rp.cpu().numpy().copy()))
    want_nis, want_ev = _read_rows(rnis, rev)
    mgr, b, _stream = _live_manager(name, dtype, p0)
    nis, ev = _rows(TICKS)
    pose = torch.zeros((7, LD), dtype=torch.float64, device="cuda")
    qd, qp = torch.zeros((N,), dtype=torch.float64, device="cuda"), torch.zeros((N, 7), dtype=torch.float64, device="cuda")
    b.live_set_pose_output(pose)
    b.live_set_gate(gamma, nis, reacquire=(3, ev))
    h_pose = torch.empty((7, LD), dtype=torch.float64).pin_memory()
    h_qd, h_qp = torch.empty((N,), dtype=torch.float64).pin_memory(), torch.empty((N, 7), dtype=torch.float64).pin_memory()
    torch.cuda.synchronize()
    copy = torch.cuda.Stream()
    mgr.live_start_all(DT, [soa], [has], max_ticks=TICKS, idle_limit_s=3.0, query=(origin, radius, [qd], [qp]))
    reinit_seen = 0
    try:
        for s in range(TICKS):
            mgr.live_post_all(1)
            assert mgr.live_wait_all(s + 1, 5.0)
            with torch.cuda.stream(copy):
                h_pose.copy_(pose, non_blocking=True)
                h_qd.copy_(qd, non_blocking=True)
                h_qp.copy_(qp, non_blocking=True)
            copy.synchronize()
            np.testing.assert_array_equal(h_pose.numpy()[:, :N].T, want[s][0], err_msg="poses of tick %d" % s)
            np.testing.assert_array_equal(h_qd.numpy(), want[s][1], err_msg="query delta of tick %d" % s)
            np.testing.assert_array_equal(h_qp.numpy(), want[s][2], err_msg="query pose of tick %d" % s)
            reinit_seen += int((want_ev[s] & 0x80).astype(bool).sum())
    finally:
        served = mgr.live_stop_all()
    assert served == TICKS and reinit_seen >= 40
    got_nis, got_ev = _read_rows(nis, ev)
    np.testing.assert_array_equal(got_nis, want_nis)
    np.testing.assert_array_equal(got_ev, want_ev)
    gx, wx = mgr.get_state_batch(IDS), ref_mgr.get_state_batch(IDS)
    np.testing.assert_array_equal(gx[0], wx[0])
    np.testing.assert_array_equal(gx[1], wx[1])
    ref_mgr.close(); mgr.close()


def test_a_manager_with_two_models_resident_together(models):
    """7.  Angular rates and angular velocities, f64, 203 targets each, the gate set on both batches: the live_start_all session
    against target_manager_step_sequence_all_reacquire, bit for bit."""
    parts, dtype = ["angular_rates", "angular_velocities"], "f64"
    gamma = gate_ref.CHI2_99[6]

    def build(stream=None):
        mgr = te.TargetManager(dtype=dtype)
        if stream is not None:
            mgr.set_stream(stream.cuda_stream)
        soas, hass = [], []
        for k, name in enumerate(parts):
            mdl = models[name]
            p0, meas, mask, soa, has = _tensors(name, dtype)
            mgr.init_batch(IDS + 1000 * k, DT, 0.0, p0, type=mdl["model"], Q=mdl["Q"], R=mdl["R"], P0=mdl["P"])
            soas.append(soa); hass.append(has)
        rows = [_rows(TICKS) for _ in parts]
        return mgr, soas, hass, rows

    def collect(mgr, rows):
        out = []
        for k, b in enumerate(mgr.batches()):
            ids = IDS + 1000 * k
            d = _state(mgr, b, ids)
            d["nis"], d["events"] = _read_rows(*rows[k])
            out.append(d)
        return out
    ref_mgr, soas, hass, rrows = build()
    ref_mgr.step_sequence_all(DT, soas, hass, use_graph=0, innov=[(r[0], None) for r in rrows], gate=gamma, reacquire=[(3, r[1]) for r in rrows])
    want = collect(ref_mgr, rrows)
    ref_mgr.close()
    stream = torch.cuda.Stream()
    mgr, soas, hass, rows = build(stream)
    for b, r in zip(mgr.batches(), rows):
        b.live_set_gate(gamma, r[0], reacquire=(3, r[1]))
    torch.cuda.synchronize()
    mgr.live_start_all(DT, soas, hass, max_ticks=TICKS, idle_limit_s=3.0)
    try:
        mgr.live_post_all(1)
        assert mgr.live_wait_all(1, 5.0)
        mgr.live_post_all(TICKS - 1)
        assert mgr.live_wait_all(TICKS, 5.0)
    finally:
        served = mgr.live_stop_all()
    assert served == TICKS
    got = collect(mgr, rows)
    for k, name in enumerate(parts):
        _same(got[k], want[k], "%s in a two-model session" % name)
        assert ((got[k]["events"] & 0x80) != 0).sum() >= 40
    mgr.close()


def test_refusals(models):
    """8.  The refusal list one by one: a negative code with the reason, nothing launched or changed -- after each a plain session on
    the same batch still runs and equals single ticks.  With a gate set, live_capacity is at most the ungated figure and at least N."""
    import ctypes as C
    from target_estimation_amd import capi
    name, dtype = "uniform_velocity", "f64"
    p0, meas, mask, soa, has = _tensors(name, dtype)
    mgr, b, _stream = _live_manager(name, dtype, p0)
    ref_mgr = _manager(name, dtype)
    _init(ref_mgr, IDS, p0)
    rb = ref_mgr.batches()[0]
    nis, ev = _rows(2)
    lib, h = b._lib, b._h
    state = {"tick": 0}

    def plain_session_still_runs(what):
        s = state["tick"] % (TICKS - 1)
        state["tick"] += 2
        b.live_start(DT, soa[s:s + 2], has[s:s + 2], max_ticks=2, idle_limit_s=3.0)
        try:
            b.live_post(2)
            assert b.live_wait(2, 5.0), what
        finally:
            assert b.live_stop() == 2
        for k in (s, s + 1):
            rb.step(DT, soa[k], has[k])
        g, w = mgr.get_state_batch(IDS), ref_mgr.get_state_batch(IDS)
        np.testing.assert_array_equal(g[0], w[0], err_msg=what)
        np.testing.assert_array_equal(g[1], w[1], err_msg=what)
        assert (torch.isnan(nis).all() and (ev == PAD).all()).item(), what + ": a refused gate wrote rows"

    def stream(ptr=nis.data_ptr(), innov=None, ld=LD, stride=LD, ring=2):
        s = capi.InnovStream()
        s.nis_dev, s.innov_dev, s.ld, s.nis_tick_stride, s.ring_ticks = ptr, innov, ld, stride, ring
        return s

    def policy(k=3, ptr=ev.data_ptr(), ld=LD, stride=LD, ring=2):
        r = capi.Reacquire()
        r.max_rejects, r.event_dev, r.ld, r.tick_stride, r.ring_ticks = k, ptr, ld, stride, ring
        return r
    plain_cap = b.live_capacity
    refusals = [
        ("nis_max < 0", -1.0, stream(), None, "nis_max"),
        ("nis_max NaN", float("nan"), stream(), None, "nis_max"),
        ("a gate without nis_dev", 9.0, stream(ptr=None), None, "nis_dev"),
        ("innov_dev != NULL", 9.0, stream(innov=nis.data_ptr()), None, "innov_dev"),
        ("ld < size", 9.0, stream(ld=N - 1, stride=N - 1), None, "ld"),
        ("a stride in (0, ld)", 9.0, stream(stride=LD - 1), None, "stride"),
        ("a negative stride", 9.0, stream(stride=-LD), None, "stride"),
        ("ring_ticks < 0", 9.0, stream(ring=-1), None, "ring"),
        ("max_rejects < 0", 9.0, stream(), policy(k=-1), "max_rejects"),
        ("max_rejects > 127", 9.0, stream(), policy(k=128), "max_rejects"),
        ("event rows: ld < size", 9.0, stream(), policy(ld=N - 1, stride=N - 1), "ld"),
        ("event rows: a stride in (0, ld)", 9.0, stream(), policy(stride=LD - 1), "stride"),
        ("event rows: ring_ticks < 0", 9.0, stream(), policy(ring=-1), "ring"),
        ("a policy without a gate", 0.0, stream(), policy(), "needs the gate"),
        ("a policy without NIS rows", 9.0, None, policy(), "needs the gate"),
    ]
    for what, nis_max, s, r, reason in refusals:
        rc = lib.target_batch_live_set_gate(h, nis_max, None if s is None else C.byref(s), None if r is None else C.byref(r))
        err = lib.target_manager_last_error().decode()
        assert rc < 0 and reason in err, (what, rc, err)
        assert b.live_capacity == plain_cap, what + ": a refused gate changed the capacity"
        plain_session_still_runs(what)
    # a batch that keeps measured poses
    mgr.set_keep_measurement(True); ref_mgr.set_keep_measurement(True)
    with pytest.raises(RuntimeError, match="keeps measured poses"):
        b.live_set_gate(9.0, nis)
    mgr.set_keep_measurement(False); ref_mgr.set_keep_measurement(False)
    plain_session_still_runs("keeps measured poses")
    # a batch that grew past ld since the call: refused at live_start, as the pose output is
    small = torch.full((1, N), float("nan"), dtype=torch.float64, device="cuda")
    b.live_set_gate(9.0, small)
    assert N <= b.live_capacity <= plain_cap
    extra = np.array([4_000_001], dtype=np.uint32)
    mgr.init_batch(extra, DT, mgr.getTime(int(IDS[0])), p0[:1]); ref_mgr.init_batch(extra, DT, ref_mgr.getTime(int(IDS[0])), p0[:1])
    with pytest.raises(RuntimeError, match="grew since live_set_gate"):
        b.live_start(DT, soa[:2], None, max_ticks=2, idle_limit_s=3.0)
    assert mgr.erase(4_000_001) and ref_mgr.erase(4_000_001)
    b.live_set_gate(0.0, None)                     # off again: sessions are exactly the plain ones
    assert b.live_capacity == plain_cap
    plain_session_still_runs("after the gate was switched off")
    # everything live_start refuses: a batch without resident kernels has no gated one either
    dense = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=3)
    _init(dense, IDS, p0)
    db = dense.batches()[0]
    assert db.live_gate_served == 0
    with pytest.raises(RuntimeError, match="no gated resident kernel"):
        db.live_set_gate(9.0, nis)
    dense.close()
    assert lib.target_batch_live_gate_served(None) == -1
    ref_mgr.close(); mgr.close()


def test_too_many_initial_covariances_refuse_a_policy_that_re_initialises(models):
    """8, continued.  A batch that no longer keeps its initial covariances: max_rejects > 0 is refused, K = 0 and gate only are not."""
    name, dtype = "uniform_velocity", "f64"
    mdl = models[name]
    n = 4200                                       # more distinct P0 than the batch's table keeps
    rng = np.random.default_rng(3)
    p0 = np.concatenate([rng.normal(0, 2.0, (n, 3)), np.tile([0, 0, 0, 1.0], (n, 1))], 1)
    P0 = np.asarray(mdl["P"], float)[None] * (1.0 + np.arange(n)[:, None, None] * 1e-3)
    mgr = te.TargetManager(dtype=dtype)
    mgr.init_batch(np.arange(n, dtype=np.uint32), DT, 0.0, p0, type=mdl["model"], Q=mdl["Q"], R=mdl["R"], P0=P0)
    b = mgr.batches()[0]
    nis = torch.full((1, n), float("nan"), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="no longer keeps its initial covariances"):
        b.live_set_gate(9.0, nis, reacquire=(3, None))
    b.live_set_gate(9.0, nis, reacquire=(0, None))
    b.live_set_gate(9.0, nis)
    mgr.close()
