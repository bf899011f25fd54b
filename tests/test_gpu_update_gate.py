"""The update policy of the by-id and one-target paths (target_manager_set_update_gate, target_manager_update_meas_batch_gated;
set_update_gate / update_batch(gated=True) in manager.py): the NIS gate and the re-acquisition of the dense calls, reached with
one call by a caller of the reference's own symbols.

Every state comparison is bit equality.  The defining properties: a gated by-id run equals an ungated by-id run with the mask
has & (0 <= nis <= gamma) from the gated run's own output, and a by-id run under (gamma, K) equals the dense
Batch.step_sequence(gate=, reacquire=) run tick by tick.  The streams are those of tests/gate_ref.py and tests/reacquire_ref.py
(203 targets: three full tiles and one of 11; 20 ticks; dt 0.004); ids are passed in a fixed random permutation so that a
wavefront's lanes land in different tiles.  tests/test_update_gate_reference.py holds the conditions these tests rest on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gate_ref
import oracle
import reacquire_ref as rq
from conftest import HARNESS_ORDER, model_path

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

N, TICKS, DT = rq.N, rq.TICKS, rq.DT
IDS = np.arange(N, dtype=np.uint32) * 3 + 1
PERM = np.random.default_rng(11).permutation(N)
GAMMA, K = gate_ref.GAMMA_FAR, 3


def _mgr(name, dtype="f64", lanes=0, policy=None, p0=None, ids=IDS, **kw):
    mgr = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=lanes, **kw)
    if policy is not None:
        mgr.set_update_gate(*policy)
    if p0 is not None:
        assert mgr.init_batch(ids, DT, 0.0, p0) == len(ids)
    return mgr


def _state(mgr, ids=IDS):
    x, P = mgr.get_state_batch(ids)
    nm = np.array([mgr.getNumberMeasurements(int(i)) for i in ids])
    t = np.array([mgr.getTime(int(i)) for i in ids])
    return dict(x=x, P=P, nm=nm, t=t)


def _same(a, b, what=""):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def _accepted(nis, mask, gamma):
    with np.errstate(invalid="ignore"):
        return mask.astype(bool) & (nis >= 0.0) & (nis <= gamma)


def _by_id(mgr, meas, mask, chunk=None, perm=PERM, ids=IDS):
    """the stream through update_batch(gated=True), ids permuted, `chunk` entries per call: nis, events [ticks, n] by TARGET"""
    ticks, n = mask.shape
    nis, ev = np.zeros((ticks, n)), np.zeros((ticks, n), np.uint8)
    for s in range(ticks):
        for lo in range(0, n, chunk or n):
            sel = perm[lo:lo + (chunk or n)]
            done, a, b = mgr.update_batch(ids[sel], DT, meas[s, sel], mask[s, sel], gated=True)
            assert done == len(sel)
            nis[s, sel], ev[s, sel] = a, b
    return nis, ev


def _runs(mgr, ids=IDS):
    return np.array([mgr.getRejectionRun(int(i)) for i in ids], np.uint8)


def _soa(meas_t, dtype, ld):
    """meas [n, 7] of one tick -> CUDA SoA [1, 7, ld] in the precision"""
    tdt = torch.float64 if dtype == "f64" else torch.float32
    soa = torch.zeros((1, 7, ld), dtype=tdt, device="cuda")
    soa[0, :, :meas_t.shape[0]] = torch.from_numpy(np.ascontiguousarray(meas_t.T)).to("cuda").to(tdt)
    return soa


# every model x {f64, f32} x lanes {0, 201, 301}, plus f64 with shared_axes=False (f64 0 / 301 start in the shared-axes form)
GATE_CASES = [(m, d, g, None) for m in HARNESS_ORDER for d in ("f64", "f32") for g in (0, 201, 301)] + [(m, "f64", 0, False) for m in HARNESS_ORDER]


@pytest.mark.parametrize("name,dtype,lanes,shared", GATE_CASES)
def test_gated_equals_masked_by_id(name, dtype, lanes, shared):
    """Test 1: manager A under (chi-square 0.99, max_rejects -1) through update_batch(gated=True) per tick; manager B without a
    policy through update_batch with has & (0 <= nis <= gamma) from A's output: states, counters and times bit-equal; every
    rejected pair has nis > gamma or NaN; no event byte; the rejection runs untouched."""
    gamma = gate_ref.CHI2_99[gate_ref.m_of(name)]
    p0, meas, mask, _, _ = gate_ref.stream(name)
    kw = {} if shared is None else dict(shared_axes=shared)
    A, B = _mgr(name, dtype, lanes, (gamma, -1), p0, **kw), _mgr(name, dtype, lanes, None, p0, **kw)
    assert A.get_update_gate(name) == (gamma, -1) and B.get_update_gate(name) == (0.0, -1)
    assert A.update_gate_served(name) is True
    if shared is not None or (dtype == "f64" and lanes in (0, 301)):
        assert bool(A.batches()[0].shared_axes) == (shared is None)
    nis, ev = _by_id(A, meas, mask)
    acc = _accepted(nis, mask, gamma)
    for s in range(TICKS):
        assert B.update_batch(IDS[PERM], DT, meas[s, PERM], acc[s, PERM].astype(np.uint8)) == N
    _same(_state(A), _state(B), "gated / masked")
    has = mask.astype(bool)
    assert (nis[~has] == -1.0).all() and (nis[has] >= 0.0).all()
    rejected = has & ~acc
    print("%s %s %d: %d of %d rejected" % (name, dtype, lanes, rejected.sum(), has.sum()))
    assert rejected.sum() >= 50 and acc.sum() >= 1000
    assert not ev.any() and not _runs(A).any()
    A.close(); B.close()


REACQ_CASES = [(m, d, g) for m in HARNESS_ORDER for d, g in (("f64", 0), ("f32", 0), ("f64", 201), ("f32", 201))]


def _expected_counts(name):
    want = rq.reference(name, GAMMA, K)
    init = (want["event"] & 0x80) != 0
    return int(init.sum()), int(((want["event"] != 0) & ~init).sum()), int((want["run"] != 0).sum())


@pytest.mark.parametrize("name,dtype,lanes", REACQ_CASES)
def test_by_id_equals_dense(name, dtype, lanes):
    """Test 2: policy (300, K = 3) on reacquire_ref.stream; A steps by id (permuted), C with Batch.step_sequence(gate=300,
    reacquire=3).  After every tick NIS by target, event bytes, rejection runs, x and P are bit-equal; the event counts are those
    of the CPU twin, so re-initialisations were reached."""
    p0, meas, mask, _, _ = rq.stream(name)
    A, C = _mgr(name, dtype, lanes, (GAMMA, K), p0), _mgr(name, dtype, lanes, None, p0)
    b, ld = C.batches()[0], N + 5
    nis_d = torch.zeros((1, ld), dtype=torch.float64, device="cuda")
    ev_d = torch.zeros((1, ld), dtype=torch.uint8, device="cuda")
    events = np.zeros((TICKS, N), np.uint8)
    for s in range(TICKS):
        nis, ev = _by_id(A, meas[s:s + 1], mask[s:s + 1])
        b.step_sequence(DT, _soa(meas[s], dtype, ld), torch.from_numpy(mask[s:s + 1].copy()).cuda(), innov=(nis_d, None), gate=GAMMA,
                        reacquire=(K, ev_d))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(nis[0], nis_d.cpu().numpy()[0, :N], err_msg="NIS, tick %d" % s)
        np.testing.assert_array_equal(ev[0], ev_d.cpu().numpy()[0, :N], err_msg="events, tick %d" % s)
        np.testing.assert_array_equal(_runs(A), b.rejection_runs(), err_msg="runs, tick %d" % s)
        xa, Pa = A.get_state_batch(IDS)
        xc, Pc = C.get_state_batch(IDS)
        np.testing.assert_array_equal(xa, xc, err_msg="x, tick %d" % s)
        np.testing.assert_array_equal(Pa, Pc, err_msg="P, tick %d" % s)
        events[s] = ev[0]
    init = (events & 0x80) != 0
    got = (int(init.sum()), int(((events != 0) & ~init).sum()), int((_runs(A) != 0).sum()))
    print(name, dtype, lanes, "re-initialisations, rejections without, non-zero final runs:", got)
    assert got == _expected_counts(name) and got[0] >= 1 and got[1] >= 1 and got[2] >= 1
    A.close(); C.close()


def _policy_run(name, dtype, chunk=None, lanes=0):
    p0, meas, mask, _, _ = rq.stream(name)
    A = _mgr(name, dtype, lanes, (GAMMA, K), p0)
    nis, ev = _by_id(A, meas, mask, chunk)
    out = dict(_state(A), nis=nis, ev=ev, runs=_runs(A))
    A.close()
    return out


@pytest.mark.parametrize("name,dtype", [("angular_rates", "f64"), ("uniform_velocity", "f32")])
def test_queue_flush_sizes(name, dtype):
    """Test 3, the queue: flushes of 1, 64, 65 and 203 entries (one lane; one wavefront, the queue block behind the BAR; two
    wavefronts with the wavefront counter; four) leave the same bits and report the same NIS and events."""
    whole = _policy_run(name, dtype)
    assert ((whole["ev"] & 0x80) != 0).sum() >= 1
    for chunk in (1, 64, 65):
        _same(whole, _policy_run(name, dtype, chunk), "flushes of %d" % chunk)


def _bulk_routes_case():
    """(child process, TE_SMALL_BATCH_QUEUE=0) the host indexed path and the whole-batch path against the dense call, and the
    device-resolved path (>= 8192 ids) against the host indexed path"""
    for name, dtype in (("angular_velocities", "f64"), ("uniform_acceleration", "f32")):
        p0, meas, mask, _, _ = rq.stream(name)
        for perm in (PERM, np.arange(N)):   # permuted: host look-up + indexed launch; slot order: the whole batch, dense kernels
            A, C = _mgr(name, dtype, 0, (GAMMA, K), p0), _mgr(name, dtype, 0, None, p0)
            b, ld = C.batches()[0], N
            nis_d = torch.zeros((TICKS, ld), dtype=torch.float64, device="cuda")
            ev_d = torch.zeros((TICKS, ld), dtype=torch.uint8, device="cuda")
            nis, ev = _by_id(A, meas, mask, perm=perm)
            tdt = torch.float64 if dtype == "f64" else torch.float32
            soa = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).cuda().to(tdt).contiguous()
            b.step_sequence(DT, soa, torch.from_numpy(mask.copy()).cuda(), innov=(nis_d, None), gate=GAMMA, reacquire=(K, ev_d))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(nis, nis_d.cpu().numpy())
            np.testing.assert_array_equal(ev, ev_d.cpu().numpy())
            np.testing.assert_array_equal(_runs(A), b.rejection_runs())
            assert ((ev & 0x80) != 0).sum() >= 1
            xa, Pa = A.get_state_batch(IDS)
            xc, Pc = C.get_state_batch(IDS)
            np.testing.assert_array_equal(xa, xc)
            np.testing.assert_array_equal(Pa, Pc)
            A.close(); C.close()
    # device-resolved: one uniform-velocity batch of 8300 targets, 8200 shuffled ids + 5 unknown ones, 3 ticks; the twin takes the
    # same entries in two calls of 4100 (+ the unknown ones), which the host table resolves
    n, m = 8300, 8200
    rng = np.random.default_rng(3)
    ids = np.arange(n, dtype=np.uint32) * 2 + 7
    p0 = np.concatenate([rng.uniform(-5, 5, (n, 3)), np.tile([0, 0, 0, 1.0], (n, 1))], 1)
    sel = rng.permutation(n)[:m]
    call_ids = np.concatenate([ids[sel], np.array([0, 2, 4, 6, 4000000000], np.uint32)])
    order = rng.permutation(m + 5)
    call_ids = call_ids[order]
    known = np.isin(call_ids, ids)
    row = {int(i): k for k, i in enumerate(ids)}
    A, B = _mgr("uniform_velocity", "f64", 0, (GAMMA, 2), p0, ids), _mgr("uniform_velocity", "f64", 0, (GAMMA, 2), p0, ids)
    total_init = 0
    for s in range(3):
        meas = np.zeros((m + 5, 7)); meas[:, 6] = 1.0
        for e, i in enumerate(call_ids):
            if known[e]:
                meas[e, :3] = p0[row[int(i)], :3] + rng.normal(0, 0.01, 3)
        out = rng.random(m + 5) < 0.3          # +0.5 m on x: rejected; on two ticks running: re-initialised
        meas[out, 0] += 0.5
        has = (rng.random(m + 5) < 0.9).astype(np.uint8)
        done, nis, ev = A.update_batch(call_ids, DT, meas, has, gated=True)
        assert done == m
        assert (nis[~known] == -2.0).all() and (ev[~known] == 0).all()
        assert (nis[known & (has == 0)] == -1.0).all() and (nis[known & (has != 0)] >= 0.0).all()
        nis2, ev2 = np.zeros(m + 5), np.zeros(m + 5, np.uint8)
        for lo, hi in ((0, 4100), (4100, m + 5)):
            d2, nis2[lo:hi], ev2[lo:hi] = B.update_batch(call_ids[lo:hi], DT, meas[lo:hi], has[lo:hi], gated=True)
        np.testing.assert_array_equal(nis, nis2)
        np.testing.assert_array_equal(ev, ev2)
        total_init += int(((ev & 0x80) != 0).sum())
    assert total_init >= 100
    _same(_state(A, ids[::41]), _state(B, ids[::41]), "device-resolved / host indexed")
    xa, Pa = A.get_state_batch(ids)
    xb, Pb = B.get_state_batch(ids)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(Pa, Pb)
    untouched = np.setdiff1d(np.arange(n), sel)[:50]
    _same(_state(A, ids[untouched]), {k: v for k, v in _state(B, ids[untouched]).items()})
    assert (np.array([A.getTime(int(i)) for i in ids[untouched]]) == 0.0).all()
    A.close(); B.close()
    print("bulk routes ok")


def test_bulk_routes():
    """Test 3, the other routes, with the queue path switched off (TE_SMALL_BATCH_QUEUE=0, read once per process: a child)."""
    env = dict(os.environ, TE_SMALL_BATCH_QUEUE="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_update_gate as t; t._bulk_routes_case()"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "bulk routes ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


@pytest.mark.parametrize("name,dtype", [("angular_velocities", "f64"), ("uniform_acceleration", "f32")])
def test_one_target_symbols(name, dtype):
    """Test 4: 40 targets stepped one update(id, dt, meas) at a time under the policy equal the batch call; getRejectionRun
    follows.  Two targets with different dt in one flush equal the same steps flushed separately."""
    p0, meas, mask, _, _ = rq.stream(name)
    sel = np.sort(np.concatenate([rq.JUMPED[:12], np.setdiff1d(np.arange(N), rq.JUMPED)[:28]]))
    ids = IDS[sel]
    A, B = _mgr(name, dtype, 0, (GAMMA, K), p0[sel], ids), _mgr(name, dtype, 0, (GAMMA, K), p0[sel], ids)
    events = np.zeros((TICKS, len(sel)), np.uint8)
    for s in range(TICKS):
        for k, j in enumerate(sel):
            A.update(int(ids[k]), DT, meas[s, j] if mask[s, j] else None)
        _, _, events[s] = B.update_batch(ids, DT, meas[s, sel], mask[s, sel], gated=True)
        np.testing.assert_array_equal(_runs(A, ids), _runs(B, ids), err_msg="runs, tick %d" % s)
    assert ((events & 0x80) != 0).sum() >= 1 and _runs(A, ids).any()
    _same(_state(A, ids), _state(B, ids), "one at a time / batch")
    # two targets, two dt, one flush (A) / two flushes (B: a getter in between)
    a, b2 = int(ids[0]), int(ids[1])
    y = meas[TICKS - 1, sel]
    for mgr, split in ((A, False), (B, True)):
        mgr.update(a, 0.004, y[0])
        if split:
            mgr.getTime(a)
        mgr.update(b2, 0.007, y[1] + np.array([0.5, 0, 0, 0, 0, 0, 0]))
    _same(_state(A, ids), _state(B, ids), "dt per entry")
    np.testing.assert_array_equal(_runs(A, ids), _runs(B, ids))
    assert A.getTime(b2) - A.getTime(a) == pytest.approx(0.003, abs=1e-12)
    A.close(); B.close()


@pytest.mark.parametrize("name,dtype", [("angular_rates", "f64"), ("angular_velocities", "f32"), ("uniform_velocity", "f64")])
def test_nan_and_zero_quaternion(name, dtype):
    """Test 5: a NaN measurement and (angular models) a zero quaternion are rejected and counted, never re-initialise (K = 1: any
    finite rejected measurement would), and no NaN reaches a record."""
    p0, meas, mask, _, _ = gate_ref.stream(name)
    n = 70
    ids = IDS[:n]
    A = _mgr(name, dtype, 0, (GAMMA, 1), p0[:n], ids)
    bad = np.zeros(n, bool)
    bad[[3, 17, 64, 69]] = True
    zero_q = np.zeros(n, bool)
    if gate_ref.m_of(name) == 6:
        zero_q[[5, 66]] = True
    for s in range(4):
        y = meas[s, :n].copy()
        y[bad, 1] = np.nan
        y[zero_q, 3:7] = 0.0
        _, nis, ev = A.update_batch(ids[::-1], DT, y[::-1], None, gated=True)
        nis, ev = nis[::-1], ev[::-1]
        assert np.isnan(nis[bad | zero_q]).all()
        np.testing.assert_array_equal(ev[bad | zero_q], s + 1)       # rejected, counted, not re-initialised
    runs = _runs(A, ids)
    np.testing.assert_array_equal(runs[bad | zero_q], 4)
    st = _state(A, ids)
    assert np.isfinite(st["x"]).all() and np.isfinite(st["P"]).all()
    assert (st["nm"][bad | zero_q] == 0).all()
    A.close()


def test_an_id_twice_in_one_call():
    """Test 6: an id named twice in one call is two consecutive gated steps (the queue flushes ahead of the second one)."""
    name = "uniform_acceleration"
    p0, meas, mask, _, _ = rq.stream(name)
    A, B = _mgr(name, "f64", 0, (GAMMA, 2), p0), _mgr(name, "f64", 0, (GAMMA, 2), p0)
    twice = np.concatenate([PERM, PERM[:30]])
    for s in range(0, 12, 2):
        y = np.concatenate([meas[s, PERM], meas[s + 1, PERM[:30]] + np.array([0.5, 0, 0, 0, 0, 0, 0])])
        done, nis, ev = A.update_batch(IDS[twice], DT, y, None, gated=True)
        assert done == N + 30
        _, n1, e1 = B.update_batch(IDS[PERM], DT, y[:N], None, gated=True)
        _, n2, e2 = B.update_batch(IDS[PERM[:30]], DT, y[N:], None, gated=True)
        np.testing.assert_array_equal(nis, np.concatenate([n1, n2]))
        np.testing.assert_array_equal(ev, np.concatenate([e1, e2]))
    assert ((ev & 0x80) != 0).sum() >= 1
    _same(_state(A), _state(B), "twice in one call")
    np.testing.assert_array_equal(_runs(A), _runs(B))
    A.close(); B.close()


def test_off_is_off():
    """Test 7: set, then clear (nis_max = 0): bit-equal to a manager that never had a policy; the gated call reports nothing."""
    name = "angular_rates"
    p0, meas, mask, _, _ = gate_ref.stream(name)
    A, B = _mgr(name, "f64", 0, (5.0, 3), p0), _mgr(name, "f64", 0, None, p0)
    A.set_update_gate(0.0)
    assert A.get_update_gate(name) == (0.0, -1)
    for s in range(6):
        done, nis, ev = A.update_batch(IDS[PERM], DT, meas[s, PERM], mask[s, PERM], gated=True)
        assert done == N and (nis == -1.0).all() and not ev.any()
        A.update(int(IDS[0]), DT, meas[s, 0])
        B.update_batch(IDS[PERM], DT, meas[s, PERM], mask[s, PERM])
        B.update(int(IDS[0]), DT, meas[s, 0])
    _same(_state(A), _state(B), "off")
    assert not _runs(A).any()
    A.close(); B.close()


def _refused(mgr, ids, meas, what, groups=None):
    """groups: the ids batch by batch (get_state_batch reads one batch's state size at a time)"""
    groups = groups or [ids]
    before = [_state(mgr, g) for g in groups]
    with pytest.raises(RuntimeError, match="gate"):
        mgr.update_batch(ids, DT, meas, None, gated=True)
    with pytest.raises(RuntimeError, match="gate"):
        mgr.update_batch(ids, DT, meas)
    for g, was in zip(groups, before):
        _same(was, _state(mgr, g), what)


def test_refusals(models):
    """Test 8: every refused case returns a negative code with a message naming the gate, and state and time of every target of
    the call are unchanged -- those of a served batch named in the same call included."""
    name = "uniform_velocity"
    p0, meas, _, _, _ = gate_ref.stream(name)
    mgr = _mgr(name, "f64", 0, None, p0[:40], IDS[:40])
    for bad in ((-1.0, -1), (float("nan"), -1), (5.0, -2), (5.0, 128), (0.0, 0), (0.0, 3)):
        with pytest.raises(RuntimeError, match="gate"):
            mgr.set_update_gate(*bad)
    with pytest.raises(RuntimeError, match="gate"):
        mgr.set_update_gate(5.0, -1, type=7)
    assert mgr.get_update_gate(name) == (0.0, -1)
    # a coupled-matrix batch (dense layout) of another model next to the served one, named in the same call
    ua = models["uniform_acceleration"]
    Q = np.array(ua["Q"], float).copy()
    Q[0, 1] = Q[1, 0] = 1e-6
    ids_ua = np.arange(900, 910, dtype=np.uint32)
    p0u = gate_ref.stream("uniform_acceleration")[0][:10]
    assert mgr.init_batch(ids_ua, DT, 0.0, p0u, type=ua["model"], Q=Q, R=ua["R"], P0=ua["P"]) == 10
    mgr.set_update_gate(GAMMA, 3)
    assert mgr.update_gate_served("uniform_velocity") is True and mgr.update_gate_served("uniform_acceleration") is False
    assert mgr.update_gate_served("angular_rates") is None
    both = np.concatenate([IDS[:40], ids_ua])
    _refused(mgr, both, np.concatenate([meas[0, :40], p0u]), "coupled matrices", [IDS[:40], ids_ua])
    mgr.update(int(ids_ua[0]), DT, p0u[0])          # the void one-target symbol: last_error, nothing stepped
    assert "gate" in te.capi.last_error() and mgr.getTime(int(ids_ua[0])) == 0.0
    done, nis, ev = mgr.update_batch(IDS[:40], DT, meas[0, :40], None, gated=True)    # the served batch alone: served
    assert done == 40 and (nis >= 0).all()
    mgr.close()
    # two (Q, R) classes
    uv = models[name]
    mgr = te.TargetManager(dtype="f64")
    Q2 = np.stack([uv["Q"], np.array(uv["Q"]) * 2.0])
    R2, P2 = np.stack([uv["R"], uv["R"]]), np.stack([uv["P"], uv["P"]])
    assert mgr.init_batch_classes(IDS[:40], DT, 0.0, p0[:40], uv["model"], Q2, R2, P2, np.arange(40) % 2) == 40
    mgr.set_update_gate(GAMMA)
    assert mgr.update_gate_served(name) is False
    _refused(mgr, IDS[:40], meas[0, :40], "two classes")
    mgr.close()
    # measured-pose rows
    mgr = _mgr(name, "f64", 0, (GAMMA, -1), p0[:40], IDS[:40])
    mgr.set_keep_measurement(True)
    assert mgr.update_gate_served(name) is False
    _refused(mgr, IDS[:40], meas[0, :40], "keep_measurement")
    mgr.close()


def test_shared_form_with_promoted_tiles():
    """Test 9: dense ticks until tiles are uniform, then gated by-id steps (which see settled tiles): bit-equal to the
    shared_axes=False twin."""
    name = "uniform_acceleration"
    p0, meas, mask, _, _ = rq.stream(name)
    A, B = _mgr(name, "f64", 0, (GAMMA, K), p0), _mgr(name, "f64", 0, (GAMMA, K), p0, shared_axes=False)
    assert A.batches()[0].shared_axes and not B.batches()[0].shared_axes
    for mgr in (A, B):
        b = mgr.batches()[0]
        for s in range(4):
            b.step(DT, _soa(meas[s], "f64", N)[0])
    assert A.batches()[0].uniform_tiles > 0 and B.batches()[0].uniform_tiles == 0
    for s in range(4, TICKS):
        na, ea = _by_id(A, meas[s:s + 1], mask[s:s + 1])
        nb, eb = _by_id(B, meas[s:s + 1], mask[s:s + 1])
        np.testing.assert_array_equal(na, nb)
        np.testing.assert_array_equal(ea, eb)
    assert A.batches()[0].shared_axes
    _same(_state(A), _state(B), "shared / plain")
    np.testing.assert_array_equal(_runs(A), _runs(B))
    assert _runs(A).any()
    A.close(); B.close()


def test_two_shards_equal_one():
    """Test 10: a manager over two shards equals the one-shard manager, outputs in the caller's order, unknown ids -2 / 0."""
    name = "angular_rates"
    p0, meas, mask, _, _ = rq.stream(name)
    A, B = _mgr(name, "f64", 0, None, None, devices=[0, 0]), _mgr(name, "f64", 0, None, None)
    for mgr in (A, B):
        mgr.set_update_gate(GAMMA, K)
        assert mgr.init_batch(IDS, DT, 0.0, p0) == N
    assert A.num_shards == 2 and len({A.shard_of(int(i)) for i in IDS}) == 2
    ids = np.concatenate([IDS[PERM], np.array([0, 2], np.uint32)])
    sel = np.concatenate([PERM, [0, 1]])
    any_init = 0
    for s in range(TICKS):
        y, h = meas[s, sel], mask[s, sel]
        da, na, ea = A.update_batch(ids, DT, y, h, gated=True)
        db, nb, eb = B.update_batch(ids, DT, y, h, gated=True)
        assert da == db == N and (na[-2:] == -2.0).all() and not ea[-2:].any()
        np.testing.assert_array_equal(na, nb)
        np.testing.assert_array_equal(ea, eb)
        any_init += int(((ea & 0x80) != 0).sum())
    assert any_init >= 1
    _same(_state(A), _state(B), "two shards / one")
    np.testing.assert_array_equal(_runs(A), _runs(B))
    A.close(); B.close()


def test_ingest_tick_under_the_policy(models):
    """Test 11: a short target_ingest_tick run with an outlier frame under the policy equals the same run without a policy in
    which that frame carried no new measurement: the outlier is not folded in."""
    m = models["uniform_velocity"]
    rng = np.random.default_rng(9)
    frames = [(k, i, np.concatenate([np.array([0.1 * i, 0.0, 1.0]) + 0.5 * k * DT + rng.normal(0, 0.005, 3), [0, 0, 0, 1.0]]))
              for k in range(12) for i in (4, 9)]
    out = {}
    for policy in (True, False):
        mgr = te.TargetManager()
        if policy:
            mgr.set_update_gate(GAMMA)
        ing = te.MeasurementIngest(mgr, m["model"], m["Q"], m["R"], m["P"], expiration_time=10.0)
        for k, i, pose in frames:
            outlier = k == 7 and i == 9
            if outlier and not policy:
                ing.push(i, 50.0 + (k - 1) * DT, pose)   # the masked run: a re-sent old stamp is no new measurement (predict only)
            else:
                ing.push(i, 50.0 + k * DT, pose + (np.array([0.5, 0, 0, 0, 0, 0, 0]) if outlier else 0.0))
            if i == 9:
                ids, _ = ing.tick(DT, 50.0 + k * DT)
        out[policy] = _state(mgr, np.array([4, 9], np.uint32))
        ing.close(); mgr.close()
    _same(out[True], out[False], "ingest")
    assert out[True]["nm"][1] == out[True]["nm"][0] - 1
