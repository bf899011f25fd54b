"""Re-acquisition of lost tracks inside the gated ticks (target_batch_step_sequence_reacquire,
target_manager_step_sequence_all_reacquire; reacquire= in manager.py): every slot keeps its run of consecutive gate rejections on
the device, and on its K-th consecutive rejection a target is re-initialised from that tick's measurement with its own initial
covariance, behind the tick's step.

The defining property, held bit for bit: the feature run equals a manager stepped one tick per call with the plain gate= call,
host counters kept from the NIS rows it reads back, and erase + init by id for every target the rule re-initialises.  Numeric
checks are against the twin of tests/reacquire_ref.py; tests/test_reacquire_reference.py holds the conditions these tests rest
on (at gamma = 300 every pair is at least 10 bounds from the gate: no pair is excluded)."""
import ctypes as C

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

from test_gpu_gate import GATE_POP, _accepted, _counts, _pop_manager_plain, _pop_outliers, _writer_layout  # noqa: E402
from test_gpu_innov_stream import CASES, _bufs, _init, _manager, _pop_manager, _pop_masks, _read, _soa  # noqa: E402

N, TICKS, DT = rq.N, rq.TICKS, rq.DT
PAD = 0xEE      # what the event rows hold before a call


def _events(blocks, ld):
    return torch.full((blocks, ld), PAD, dtype=torch.uint8, device="cuda")


def _read_events(ev, n):
    torch.cuda.synchronize()
    e = ev.cpu().numpy()
    assert (e[:, n:] == PAD).all(), "an event column beyond the batch size was written"
    return e[:, :n]


def _feature(name, dtype, lanes, p0, soa, has, ids, m, ld, gamma, K, use_graph=False, splits=None, shared=None, kw=None):
    """one fresh manager over the stream through the calls with reacquire=, in the calls `splits` ([(lo, hi), ...]; default: one):
    dict of nis, nu, events [ticks, n], runs, x, P, counters, times"""
    kw = kw or {}
    mgr = _manager(name, dtype, lanes, **kw, **({} if shared is None else dict(shared_axes=shared)))
    _init(mgr, ids, p0, **kw)
    b = mgr.batches()[0]
    ticks, n = soa.shape[0], len(ids)
    bufs, ev = _bufs(ticks, m, ld), _events(ticks, ld)
    for lo, hi in splits or [(0, ticks)]:
        b.step_sequence(DT, soa[lo:hi], None if has is None else has[lo:hi], use_graph=use_graph, innov=(bufs[0][lo:hi], bufs[1][lo:hi]),
                        gate=gamma, reacquire=(K, ev[lo:hi]))
    nis, nu = _read(bufs, n)
    out = dict(nis=nis, nu=nu, events=_read_events(ev, n), runs=b.rejection_runs())
    out["x"], out["P"] = mgr.get_state_batch(ids)
    out["nm"] = _counts(mgr, ids)
    out["t"] = np.array([mgr.getTime(int(i)) for i in ids])
    out["shared"] = b.shared_axes
    np.testing.assert_array_equal(out["runs"], [mgr.getRejectionRun(int(i)) for i in ids])
    assert mgr.getRejectionRun(4000000) is None
    mgr.close()
    return out


def _host_rule(model, nis, mask, meas_t, gamma, K):
    """the rule of the contract from NIS rows [ticks, n] read back, mask [ticks, n] and the measurements as the ticks read them
    [ticks, n, 7]: events [ticks, n], runs [n]"""
    ticks, n = nis.shape
    ev, run = np.zeros((ticks, n), np.uint8), np.zeros(n, np.uint8)
    acc = _accepted(nis, mask, gamma)
    for s in range(ticks):
        for j in range(n):
            can = bool(mask[s, j]) and not acc[s, j] and rq.initial_state_is_finite(model, meas_t[s, j])
            run[j], ev[s, j], _ = rq.event_rule(int(run[j]), bool(mask[s, j]), bool(acc[s, j]), can, K)
    return ev, run


def _as_read(meas, dtype):
    """the measurements as a tick of the batch precision reads them, float64"""
    return meas.astype(np.float32).astype(np.float64) if dtype == "f32" else meas


def _emulate(name, dtype, lanes, p0, meas, mask, ids, m, gamma, K, model):
    """The emulation of test 1: one tick per call with the plain gate= call, measurement columns ordered by the current slots, host
    counters from the NIS read back, erase + init by id for every target the rule re-initialises.  Returns x, P by id, the events
    [ticks, n] and the counters [n] (columns = positions in ids)."""
    mgr = _manager(name, dtype, lanes)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    n, ticks = len(ids), meas.shape[0]
    pos = {int(i): k for k, i in enumerate(ids)}
    read = _as_read(meas, dtype)
    run, events = np.zeros(n, np.uint8), np.zeros((ticks, n), np.uint8)
    bufs = _bufs(1, m, n)
    for s in range(ticks):
        order = np.array([pos[int(i)] for i in b.slot_ids()])
        soa = _soa(meas[s:s + 1, order], dtype, n)
        has = torch.from_numpy(np.ascontiguousarray(mask[s:s + 1, order])).cuda()
        b.step_sequence(DT, soa, has, innov=bufs, gate=gamma)
        nis = _read(bufs, n)[0][0]
        acc = _accepted(nis[None], mask[s:s + 1, order], gamma)[0]
        again = []
        for k, j in enumerate(order):
            can = bool(mask[s, j]) and not acc[k] and rq.initial_state_is_finite(model, read[s, j])
            run[j], events[s, j], init = rq.event_rule(int(run[j]), bool(mask[s, j]), bool(acc[k]), can, K)
            if init:
                again.append(j)
        for j in again:
            t = mgr.getTime(int(ids[j]))
            assert mgr.erase(int(ids[j]))
            mgr.init(int(ids[j]), DT, t, read[s, j])
    x, P = mgr.get_state_batch(ids)
    mgr.close()
    return x, P, events, run


@pytest.mark.parametrize("name,dtype,lanes", CASES)
def test_reacquire_equals_erase_and_init(name, dtype, lanes):
    """Test 1, every layout, f64 and f32, at the chi-square 0.99 gate with K = 3: eager and recorded feature runs equal in every
    output; x and P by id bit-equal to the emulation; the event rows are the host rule's bytes and rejection_runs() its counters;
    the measurement counters are the accepted counts of the run's own NIS rows; every target has the same time; padding
    untouched.  Angular cases: some re-initialised target is measured on a later tick (its unwrap memory is then in use)."""
    m, ld = gate_ref.m_of(name), N + 13
    gamma = gate_ref.CHI2_99[m]
    mdl = oracle.load_model_yaml(model_path(name))["model"]
    p0, meas, mask, _, _ = rq.stream(name)
    soa, has = _soa(meas, dtype, ld), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    runs = {g: _feature(name, dtype, lanes, p0, soa, has, ids, m, ld, gamma, 3, use_graph=g) for g in (False, True)}
    for k, v in runs[False].items():
        np.testing.assert_array_equal(runs[True][k], v, err_msg="eager / recorded: " + k)
    got = runs[False]
    init = (got["events"] & 0x80) != 0
    print("%s %s %d: %d re-initialisations" % (name, dtype, lanes, init.sum()))
    assert init.sum() >= 40
    if m == 6:
        later = [(s, j) for s, j in zip(*np.nonzero(init)) if mask[s + 1:, j].any()]
        assert later, "no re-initialised target is measured on a later tick"
    ev, run = _host_rule(mdl, got["nis"], mask, _as_read(meas, dtype), gamma, 3)
    np.testing.assert_array_equal(got["events"], ev)
    np.testing.assert_array_equal(got["runs"], run)
    np.testing.assert_array_equal(got["nm"], _accepted(got["nis"], mask, gamma).sum(0))
    assert (got["t"] == got["t"][~init.any(0)][0]).all(), "a re-initialised target's clock differs"
    x, P, events, counters = _emulate(name, dtype, lanes, p0, meas, mask, ids, m, gamma, 3, mdl)
    np.testing.assert_array_equal(got["events"], events)
    np.testing.assert_array_equal(got["runs"], counters)
    np.testing.assert_array_equal(got["x"], x)
    np.testing.assert_array_equal(got["P"], P)


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_velocity", "f64", 0), ("angular_rates", "f32", 301), ("angular_velocities", "f64", 103),
                                              ("uniform_acceleration", "f32", 1)])
def test_the_runs_persist_between_calls(name, dtype, lanes):
    """Test 2: the feature run split into two calls (ticks 0-9, 10-19) and into 20 single-tick calls: every output bit-equal to the
    single call.  A plain gate= call leaves rejection_runs() unchanged."""
    m, ld = gate_ref.m_of(name), N + 13
    gamma = gate_ref.CHI2_99[m]
    p0, meas, mask, _, _ = rq.stream(name)
    soa, has = _soa(meas, dtype, ld), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    one = _feature(name, dtype, lanes, p0, soa, has, ids, m, ld, gamma, 3)
    assert ((one["events"] & 0x80) != 0).sum() >= 40 and one["runs"].any()
    for splits in ([(0, 10), (10, 20)], [(s, s + 1) for s in range(TICKS)]):
        got = _feature(name, dtype, lanes, p0, soa, has, ids, m, ld, gamma, 3, splits=splits)
        for k, v in one.items():
            np.testing.assert_array_equal(got[k], v, err_msg="%d calls: %s" % (len(splits), k))
    mgr = _manager(name, dtype, lanes)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    bufs = _bufs(TICKS, m, ld)
    b.step_sequence(DT, soa[:12], has[:12], innov=(bufs[0][:12], bufs[1][:12]), gate=gamma, reacquire=(3, None))
    before = b.rejection_runs()
    assert before.any()
    b.step_sequence(DT, soa[12:], has[12:], innov=(bufs[0][12:], bufs[1][12:]), gate=gamma)
    np.testing.assert_array_equal(b.rejection_runs(), before)
    mgr.close()


@pytest.mark.parametrize("name", ["uniform_velocity", "angular_rates", "angular_velocities"])
def test_shared_form_and_uniform_tiles(name):
    """Test 3: 137 fp64 targets with one p0 and one clean trajectory in the shared-axes form, a mask of ones: tiles promote before
    tick 8; from tick 8 on +0.5 m on x for all of slots 64..127 and 5 slots of the ragged last tile.  The whole tile is
    re-initialised on tick 10 with event 0x83 while flagged uniform; the state is bit-equal to the same stream with
    shared_axes=False; the batch is still in the form."""
    dtype, n, m, gamma = "f64", 137, gate_ref.m_of(name), gate_ref.GAMMA_FAR
    p0, meas, _, _ = ref.stream_and_reference(name, n, TICKS, 9)
    p0 = np.tile(p0[:1], (n, 1))
    meas = np.tile(meas[:, :1], (1, n, 1))
    jumped = np.r_[64:128, 128:133]
    meas[rq.JUMP_TICK:, jumped, 0] += rq.JUMP
    soa = _soa(meas, dtype, n)
    has = torch.ones((TICKS, n), dtype=torch.uint8, device="cuda")
    ids = np.arange(n, dtype=np.uint32)
    res = {}
    for shared in (True, False):
        mgr = _manager(name, dtype, shared_axes=shared)
        _init(mgr, ids, p0)
        b = mgr.batches()[0]
        assert b.shared_axes == (1 if shared else 0)
        bufs, ev = _bufs(TICKS, m, n), _events(TICKS, n)
        for lo, hi in ((0, rq.JUMP_TICK), (rq.JUMP_TICK, rq.JUMP_TICK + 2), (rq.JUMP_TICK + 2, TICKS)):
            if shared and name != "angular_velocities" and lo > 0:
                assert b.uniform_tiles > 0, "no tile is uniform ahead of tick %d: the test does not reach the settled-tile path" % lo
            b.step_sequence(DT, soa[lo:hi], has[lo:hi], innov=(bufs[0][lo:hi], bufs[1][lo:hi]), gate=gamma, reacquire=(3, ev[lo:hi]))
        events = _read_events(ev, n)
        assert b.shared_axes == (1 if shared else 0)
        rest = np.setdiff1d(np.arange(n), jumped)
        np.testing.assert_array_equal(events[rq.JUMP_TICK:rq.JUMP_TICK + 3, jumped].T, np.tile([1, 2, 0x83], (len(jumped), 1)))
        assert (events[:, rest] == 0).all() and (events[:rq.JUMP_TICK] == 0).all() and (events[rq.JUMP_TICK + 3:] == 0).all()
        res[shared] = (mgr.get_state_batch(ids), b.rejection_runs(), _counts(mgr, ids), _read(bufs, n))
        mgr.close()
    for k in (0, 1):
        np.testing.assert_array_equal(res[True][0][k], res[False][0][k])
        np.testing.assert_array_equal(res[True][3][k], res[False][3][k])
    np.testing.assert_array_equal(res[True][1], res[False][1])
    np.testing.assert_array_equal(res[True][2], res[False][2])
    assert (res[True][2][jumped] == TICKS - 3).all() and (res[True][2][np.setdiff1d(np.arange(n), jumped)] == TICKS).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_against_the_twin(name, dtype):
    """Test 4: gamma = 300, K = 3, the default layout and one whose gate is the writer's mask row: events and runs are the twin's
    exactly, no pair left out; NIS and nu within the innovation stream's bounds; the final x, P within TOL[dtype]."""
    m, ld, gamma = gate_ref.m_of(name), N + 13, gate_ref.GAMMA_FAR
    p0, meas, mask, _, _ = rq.stream(name)
    want = rq.reference(name, gamma, 3)
    soa, has = _soa(meas, dtype, ld), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    t = TOL[dtype]
    for lanes in (0, _writer_layout(name, dtype)):
        got = _feature(name, dtype, lanes, p0, soa, has, ids, m, ld, gamma, 3)
        what = "%s %s %d reacquire" % (name, dtype, lanes)
        np.testing.assert_array_equal(got["events"], want["event"], err_msg=what + ": an event differs from the twin's")
        np.testing.assert_array_equal(got["runs"], want["run"], err_msg=what)
        ref.check(got["nu"], got["nis"], want, mask, dtype, what)
        np.testing.assert_array_equal(got["nm"], want["acc"].sum(0))
        ex = np.abs(got["x"] - want["x"]).max()
        ep = max(np.abs(got["P"][j] - want["P"][j]).max() / np.abs(want["P"][j]).max() for j in range(N))
        print("%s: worst |dx| %.3g, worst |dP| / max|P| %.3g" % (what, ex, ep))
        np.testing.assert_allclose(got["x"], want["x"], atol=t["x_atol"], rtol=t["x_rtol"])
        for j in range(N):
            assert np.abs(got["P"][j] - want["P"][j]).max() <= t["P_rel"] * np.abs(want["P"][j]).max()


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_acceleration", "f32", 301), ("angular_rates", "f64", 301), ("angular_velocities", "f32", 101)])
def test_nan_and_degenerate_measurements_never_reinitialise(name, dtype, lanes):
    """Test 5: target A gets NaN on ticks 5-7 and the +0.5 m jump from tick 8: events 1, 2, 3 without the high bit, then 0x84 on
    tick 8.  Angular models: target B gets the jump and a zero quaternion on ticks 8-10: rejected and counted on each, never
    re-initialised while the quaternion is zero, re-initialised on its first measured tick with a quaternion again; no NaN reaches
    any record."""
    m, gamma = gate_ref.m_of(name), gate_ref.GAMMA_FAR
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
    soa, has = _soa(meas, dtype, N), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    got = _feature(name, dtype, lanes, p0, soa, has, ids, m, N, gamma, 3)
    ev = got["events"]
    assert (ev[:5, A] == 0).all()
    np.testing.assert_array_equal(ev[5:9, A], [1, 2, 3, 0x84])
    assert np.isnan(got["nis"][5:8, A]).all()
    if m == 6:
        assert (ev[:8, B] == 0).all()
        np.testing.assert_array_equal(ev[8:11, B], [1, 2, 3])
        assert np.isnan(got["nis"][8:11, B]).all()
        later = [s for s in range(11, TICKS) if mask[s, B]]
        assert later and ev[later[0], B] == 0x84 and (ev[11:later[0], B] == 0).all()
    assert np.isfinite(got["x"]).all() and np.isfinite(got["P"]).all()
    mdl = oracle.load_model_yaml(model_path(name))["model"]
    want_ev, want_run = _host_rule(mdl, got["nis"], mask, _as_read(meas, dtype), gamma, 3)
    np.testing.assert_array_equal(ev, want_ev)
    np.testing.assert_array_equal(got["runs"], want_run)


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_velocity", "f32", 0), ("angular_rates", "f64", 0), ("angular_velocities", "f64", 6)])
def test_k0_counts_only(name, dtype, lanes):
    """Test 6: K = 0: state, streams and counters bit-equal to the gate= call; the runs are the host rule's and reach the lock-out
    length on the jumped targets."""
    m, gamma = gate_ref.m_of(name), gate_ref.GAMMA_FAR
    p0, meas, mask, _, _ = rq.stream(name)
    soa, has = _soa(meas, dtype, N), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    got = _feature(name, dtype, lanes, p0, soa, has, ids, m, N, gamma, 0)
    mgr = _manager(name, dtype, lanes)
    _init(mgr, ids, p0)
    bufs = _bufs(TICKS, m, N)
    mgr.batches()[0].step_sequence(DT, soa, has, innov=bufs, gate=gamma)
    nis, nu = _read(bufs, N)
    x, P = mgr.get_state_batch(ids)
    for a, b in ((got["nis"], nis), (got["nu"], nu), (got["x"], x), (got["P"], P), (got["nm"], _counts(mgr, ids))):
        np.testing.assert_array_equal(a, b)
    mgr.close()
    assert not (got["events"] & 0x80).any()
    mdl = oracle.load_model_yaml(model_path(name))["model"]
    ev, run = _host_rule(mdl, got["nis"], mask, _as_read(meas, dtype), gamma, 0)
    np.testing.assert_array_equal(got["events"], ev)
    np.testing.assert_array_equal(got["runs"], run)
    since = mask[rq.JUMP_TICK:, rq.JUMPED].sum(0)
    assert (got["runs"][rq.JUMPED] >= since).all() and since.min() >= 4


@pytest.mark.parametrize("name,dtype", [("uniform_velocity", "f64"), ("angular_rates", "f32")])
def test_every_target_gets_its_own_initial_covariance(models, name, dtype):
    """Test 7: two init_batch calls with different P0 in one batch, single-tick calls: right after the tick that re-initialises it
    a target's P is the P a fresh target of its group starts with."""
    m, gamma = gate_ref.m_of(name), gate_ref.GAMMA_FAR
    mdl = models[name]
    p0, meas, mask, _, _ = rq.stream(name)
    soa, has = _soa(meas, dtype, N), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    half = N // 2 + 3
    mgr = te.TargetManager(dtype=dtype)
    for sel, scale in ((ids[:half], 1.0), (ids[half:], 2.0)):
        assert mgr.init_batch(sel, DT, 0.0, p0[sel], type=mdl["model"], Q=mdl["Q"], R=mdl["R"], P0=scale * mdl["P"]) == len(sel)
    assert len(mgr.batches()) == 1
    b = mgr.batches()[0]
    _, P_start = mgr.get_state_batch(ids)
    assert not np.array_equal(P_start[0], P_start[N - 1])
    bufs, ev = _bufs(1, m, N), _events(1, N)
    seen = np.zeros(N, bool)
    for s in range(TICKS):
        b.step_sequence(DT, soa[s:s + 1], has[s:s + 1], innov=bufs, gate=gamma, reacquire=(3, ev))
        init = (_read_events(ev, N)[0] & 0x80) != 0
        if init.any():
            _, P = mgr.get_state_batch(ids[init])
            np.testing.assert_array_equal(P, P_start[init])
            seen |= init
    assert seen[:half].any() and seen[half:].any() and seen[rq.JUMPED].all()
    mgr.close()


def _pop_jump(meas, first_tick, columns):
    for t in meas:
        t[first_tick:, 0, :columns] += rq.JUMP


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("parts,dtype,shared,plain", GATE_POP)
def test_population_tick(models, parts, dtype, shared, plain, use_graph):
    """Test 8: the one-launch population tick with per-batch policies -- batch 0 K = 3, batch 1 none -- eager and recorded: streams,
    events, runs, states and counters bit-equal to the per-batch calls, population_tick() stays true; the batch without a policy
    equals the ..._all_gated call."""
    ticks, gamma = 10, gate_ref.GAMMA_FAR
    has = _pop_masks(parts, ticks, 5)

    def fresh():
        mgr, meas, ids = (_pop_manager_plain if plain else _pop_manager)(models, parts, dtype, ticks, 77)
        _pop_outliers(meas, has, 6)
        _pop_jump(meas, 4, 40)
        return mgr, meas, ids

    mgr, meas, ids = fresh()
    want = []
    for i, b in enumerate(mgr.batches()):
        bufs, ev = _bufs(ticks, b.meas_dim, b.size + 5), _events(ticks, b.size + 5)
        b.step_sequence(DT, meas[i], has[i], innov=bufs, gate=gamma, reacquire=(3, ev) if i == 0 else None)
        out = _read(bufs, b.size)
        want.append((out, mgr.get_state_batch(ids[i]), _counts(mgr, ids[i]), _read_events(ev, b.size) if i == 0 else None, b.rejection_runs()))
    mgr.close()
    assert ((want[0][3] & 0x80) != 0).sum() >= 20, "the test does not reach a re-initialisation"
    assert not want[1][4].any()
    for policy in ([(3, "ev"), None], None):
        mgr, meas, ids = fresh()
        assert mgr.population_tick()
        bs = mgr.batches()
        bufs = [_bufs(ticks, b.meas_dim, b.size + 5) for b in bs]
        ev = _events(ticks, bs[0].size + 5)
        kw = {} if policy is None else dict(reacquire=[(3, ev), None])
        mgr.step_sequence_all(DT, meas, has_meas=has, use_graph=use_graph, innov=bufs, gate=[gamma, gamma], **kw)
        assert mgr.population_tick()
        if shared is not None:
            assert [b.shared_axes for b in bs] == [1 if shared else 0] * len(bs)
        for i, b in enumerate(bs):
            if policy is None and i == 0:
                continue    # (the gate alone: batch 0 keeps its lost targets out; batch 1 is the comparison)
            (wn, wu), (wx, wP), wc, wev, wrun = want[i]
            nis, nu = _read(bufs[i], b.size)
            np.testing.assert_array_equal(nis, wn)
            np.testing.assert_array_equal(nu, wu)
            x, P = mgr.get_state_batch(ids[i])
            np.testing.assert_array_equal(x, wx)
            np.testing.assert_array_equal(P, wP)
            np.testing.assert_array_equal(_counts(mgr, ids[i]), wc)
            if policy is not None:
                np.testing.assert_array_equal(b.rejection_runs(), wrun)
                if i == 0:
                    np.testing.assert_array_equal(_read_events(ev, b.size), wev)
        mgr.close()


def test_refusals_launch_nothing(models):
    """Test 9: a policy without a gate, K outside 0..127, malformed event rows, a batch that keeps measured poses, a batch that no
    longer keeps its initial covariances: a negative code and a message that names the re-acquisition; state, buffers and
    rejection_runs() untouched."""
    from target_estimation_amd import capi
    lib = capi.lib()
    name, dtype, n, m, gamma = "angular_rates", "f64", 100, 6, gate_ref.GAMMA_FAR
    p0, meas, mask, _ = ref.stream_and_reference(name, n, 2, 4)
    soa = _soa(meas, dtype, n)
    ids = np.arange(n, dtype=np.uint32)
    mgr = _manager(name, dtype)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    x0, P0 = mgr.get_state_batch(ids)
    nis, nu = _bufs(2, m, n)
    ev = _events(2, n)
    good = capi.InnovStream(nis.data_ptr(), nu.data_ptr(), n, n, m * n, 0)

    def call(gate, rq_c, use_graph):
        return lib.target_batch_step_sequence_reacquire(b._h, 2, DT, soa.data_ptr(), soa.stride(0), soa.stride(1), None, 0, 0, None,
                                                        C.byref(good), gate, C.byref(rq_c), use_graph)

    bad = [(0.0, capi.Reacquire(3, ev.data_ptr(), n, n, 0)), (gamma, capi.Reacquire(-1, ev.data_ptr(), n, n, 0)),
           (gamma, capi.Reacquire(128, ev.data_ptr(), n, n, 0)), (gamma, capi.Reacquire(3, ev.data_ptr(), n - 1, n, 0)),
           (gamma, capi.Reacquire(3, ev.data_ptr(), n, n - 1, 0)), (gamma, capi.Reacquire(3, ev.data_ptr(), n, -n, 0)),
           (gamma, capi.Reacquire(3, ev.data_ptr(), n, n, -1))]
    for use_graph in (0, 1):
        for gate, r in bad:
            rc = call(gate, r, use_graph)
            assert rc < 0 and "re-acquisition" in capi.last_error(), (gate, r.max_rejects, r.ld, r.tick_stride, r.ring_ticks, capi.last_error())
        rc = lib.target_batch_step_sequence_reacquire(b._h, 2, DT, soa.data_ptr(), soa.stride(0), soa.stride(1), None, 0, 0, None, None, gamma,
                                                      C.byref(capi.Reacquire(3, None, 0, 0, 0)), use_graph)
        assert rc < 0 and "gate" in capi.last_error()    # (what ..._gated refuses: a gate without a NIS row)
    with pytest.raises(RuntimeError, match="re-acquisition"):
        b.step_sequence(DT, soa, innov=(nis, nu), reacquire=(3, ev))
    with pytest.raises(RuntimeError, match="re-acquisition"):
        mgr.step_sequence_all(DT, [soa], innov=[(nis, nu)], gate=gamma, reacquire=(200, None))
    mgr.set_keep_measurement(True)
    for use_graph in (0, 1):
        assert call(gamma, capi.Reacquire(3, ev.data_ptr(), n, n, 0), use_graph) < 0 and "re-acquisition" in capi.last_error()
    mgr.set_keep_measurement(False)
    torch.cuda.synchronize()
    x1, P1 = mgr.get_state_batch(ids)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(P1, P0)
    assert torch.isnan(nis).all() and torch.isnan(nu).all() and (ev == PAD).all()
    assert not b.rejection_runs().any() and (_counts(mgr, ids) == 0).all()
    # the same batch served once the refusals are out of the way
    assert call(gamma, capi.Reacquire(3, ev.data_ptr(), n, n, 0), 0) == 0
    mgr.close()
    # more than 4096 distinct initial covariances: the batch stops keeping them
    mdl = models["uniform_velocity"]
    mgr = te.TargetManager(dtype="f64")
    k = 4100
    pose = np.tile([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], (k, 1))
    scale = 1.0 + 1e-6 * np.arange(k)
    assert mgr.init_batch_classes(np.arange(k, dtype=np.uint32), DT, 0.0, pose, mdl["model"], np.tile(mdl["Q"], (k, 1, 1)), np.tile(mdl["R"], (k, 1, 1)),
                                  mdl["P"][None] * scale[:, None, None], np.arange(k, dtype=np.uint32)) == k
    assert len(mgr.batches()) == 1
    b = mgr.batches()[0]
    assert b.size == k
    z = torch.zeros((1, 7, k), dtype=torch.float64, device="cuda")
    z[:, 6] = 1.0
    with pytest.raises(RuntimeError, match="re-acquisition"):
        b.step_sequence(DT, z, innov=_bufs(1, 3, k), gate=gamma, reacquire=(3, None))
    assert not b.rejection_runs().any()
    mgr.close()


@pytest.mark.parametrize("use_graph", [0, 1])
def test_two_shards_on_one_device(use_graph):
    """Test 10: two logical shards on device 0: the manager call with a policy on every batch leaves every target, by id, in the
    bits of the one-shard manager, with the same rejection runs and counters; the event bytes agree target by target."""
    name, m, gamma = "angular_rates", 6, gate_ref.GAMMA_FAR
    p0, meas, mask, _, _ = rq.stream(name)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    pos = {int(i): k for k, i in enumerate(ids)}
    res = []
    for devices in (None, [0, 0]):
        mgr = te.TargetManager(model_path(name), dtype="f64", devices=devices)
        assert mgr.init_batch(ids, DT, 0.0, p0) == N
        bs = mgr.batches()
        assert len(bs) == (1 if devices is None else 2)
        order = [np.array([pos[int(i)] for i in b.slot_ids()]) for b in bs]
        soa = [_soa(meas[:, o], "f64", len(o)) for o in order]
        has = [torch.from_numpy(np.ascontiguousarray(mask[:, o])).cuda() for o in order]
        bufs = [_bufs(TICKS, m, len(o)) for o in order]
        evs = [_events(TICKS, len(o)) for o in order]
        mgr.step_sequence_all(DT, soa, has_meas=has, use_graph=use_graph, innov=bufs, gate=gamma, reacquire=[(3, e) for e in evs])
        mgr.synchronize()
        events = np.zeros((TICKS, N), np.uint8)
        for o, e in zip(order, evs):
            events[:, o] = _read_events(e, len(o))
        x, P = mgr.get_state_batch(ids)
        res.append((x, P, events, np.array([mgr.getRejectionRun(int(i)) for i in ids]), _counts(mgr, ids)))
        mgr.close()
    assert ((res[0][2] & 0x80) != 0).sum() >= 24
    for a, b in zip(res[0], res[1]):
        np.testing.assert_array_equal(a, b)
