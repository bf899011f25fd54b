"""The derived outputs of every kernel path against the 50-digit attitude fixture (tests/golden/make_attitude_kat.py ->
tests/golden/attitude_kat.npz; tests/attitude_kat_ref.py): all four branches of the matrix -> quaternion rule, the quaternion's
sign, four offsets of the extrapolating getters, one to three predict-only ticks (the angular-rates pitch passes +-pi/2), the
gimbal set, omega = 0 and |omega| = 2^-40 -- in f64 and f32, behind every layout's accessors.

The rule is that of tests/test_gpu_precision.py (K = 8), per group of rows and never over the batch:

    err(kernel vs 50 digits) <= 8 * err(same-precision CPU oracle vs 50 digits, the same rows) + 8 eps(dtype)

err = max |got - want| / max(1, |want|).  STRICT rows are compared as they are, the quaternion's sign included; the rest (group
name + "~") as rotations.  tests/test_attitude_kat.py holds the oracle itself to the fixture.  `pytest -s` prints, per path and
group, the kernel's error, the faithful error and their ratio (profiles/attitude_kat_tolerances.txt keeps the MI355X table)."""
import numpy as np
import pytest

import oracle
import attitude_kat_ref as ak
from conftest import model_path
from test_gpu_crossing_cov import DENSE, LAYOUTS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

K = 8.0
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
ALL = ak.ANGULAR + ak.CONTROLS
TICKS = 3


class Rows:
    """collects the rows of one test: prints each, fails at the end with all that miss the rule"""

    def __init__(self, dtype):
        self.dtype, self.bad, self.n = dtype, [], 0

    def hold(self, path, m, view, got, same, rows=None, pose_only=False):
        e_k = ak.group_errors(m, view, got, rows, pose_only)
        e_o = ak.group_errors(m, view, same, rows, pose_only)
        floor = 8 * EPS[self.dtype]
        for g in sorted(e_k):
            print("[attitude] %-44s %-20s %-3s %-14s kernel %.2e  faithful %.2e  ratio %6.2f"
                  % (path, m.name, self.dtype, g, e_k[g], e_o[g], e_k[g] / max(e_o[g], floor)))
            self.n += 1
            if not e_k[g] <= K * e_o[g] + floor:
                self.bad.append((path, g, e_k[g], e_o[g]))

    def done(self, at_least=1):
        assert self.n >= at_least
        assert not self.bad, "kernel error over %g x faithful + 8 eps: %s" % (K, self.bad)


def _ids(n):
    return np.arange(n, dtype=np.uint32) * 3 + 5


def _manager(models, name, dtype, layout, cases=None):
    """a manager holding the fixture's cases (all, or `cases`) of one model in one layout of LAYOUTS (or "auto")"""
    m, mod = ak.Model(name), models[name]
    p0, v0, a0 = m.inputs(cases=cases)
    n = len(p0)
    ids = _ids(n)
    lanes = {"301": 301, "301shared": 301, "201": 201, "full": DENSE[name][0], "packed": DENSE[name][1], "classes": 301, "auto": 0}[layout]
    mgr = te.TargetManager(dtype=dtype, lanes_per_target=lanes, shared_axes=(layout == "301shared"))
    typ = te.MODEL_TYPES[name]
    if layout == "classes":
        Q = np.stack([mod["Q"], mod["Q"] + 1e-3 * np.eye(mod["Q"].shape[0])])
        cls = (np.arange(n) % 2).astype(np.uint32)
        assert mgr.init_batch_classes(ids, m.dt, 0.0, p0, typ, Q, np.stack([mod["R"]] * 2), np.stack([mod["P"]] * 2), cls, v0, a0) == n
    else:
        assert mgr.init_batch(ids, m.dt, 0.0, p0, v0, a0, type=typ, Q=mod["Q"], R=mod["R"], P0=mod["P"]) == n
    b = mgr.batches()[0]
    assert b.size == n
    if layout == "classes":
        assert b.num_classes == 2
    elif layout != "auto":
        assert b.shared_axes == (1 if layout == "301shared" else 0)
    return m, mgr, b, ids


def _cat(p, t, a):
    return np.concatenate([p, t, a], 1)


# ---- the getters: by id and per batch, at the target's own time and at every offset, behind every layout ---------------------------
@pytest.mark.parametrize("name,dtype,layout", [(n, d, l) for n in ALL for d in ("f64", "f32") for l in LAYOUTS
                                               if not (l == "301shared" and d == "f32")])
def test_getters(models, name, dtype, layout):
    m, mgr, b, ids = _manager(models, name, dtype, layout)
    same = ak.oracle_outputs(oracle, models, name, dtype)
    rows = Rows(dtype)
    path = "get_est_batch %s" % layout
    p, t, a, found = mgr.get_est_batch(ids)
    assert found.all()
    rows.hold(path, m, "now", _cat(p, t, a), same["now"])
    slot = np.searchsorted(ids, b.slot_ids())                 # the case in every slot of the batch
    for o, off in enumerate(m.offsets):
        sel = np.nonzero(m.offset_of == o)[0]                  # the cases whose stored offset this is
        p, t, a, found = mgr.get_est_batch(ids, t1=float(off))
        assert found.all()
        rows.hold("%s t1 %+g" % (path, off), m, "at", _cat(p, t, a)[sel], same["at"][sel], sel)
        p, t, a = (x.cpu().numpy() for x in b.get_est(t1=float(off)))
        by_case = np.empty((m.n, 19))
        by_case[slot] = _cat(p, t, a)
        rows.hold("Batch.get_est %s t1 %+g" % (layout, off), m, "at", by_case[sel], same["at"][sel], sel)
    mgr.close()
    rows.done(3)


# ---- the one-target symbols (init, getTargetPose / Twist / Acceleration) through managers of the model files: 16 strict cases per
# branch, and the gimbal set ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [(n, d) for n in ak.ANGULAR for d in ("f64", "f32")])
def test_one_target_symbols(models, name, dtype):
    m = ak.Model(name)
    same = ak.oracle_outputs(oracle, models, name, dtype)
    pick = [np.nonzero(m.strict_now & (m.branch_now == br) & ~m.gimbal)[0][:16] for br in range(4)]
    assert all(len(p) == 16 for p in pick)
    sel = np.sort(np.concatenate(pick + [np.nonzero(m.gimbal)[0]]))
    mgr = te.TargetManager(model_path(name), dtype=dtype)
    got = np.zeros((len(sel), 19))
    for j, i in enumerate(sel):          # the reference's init takes a pose only: v0 = a0 = 0, and pose7 does not depend on them
        mgr.init(int(i) + 1, m.dt, 0.0, m.p0[i])
    for j, i in enumerate(sel):
        (ok1, pose), (ok2, twist), (ok3, acc) = mgr.getTargetPose(int(i) + 1), mgr.getTargetTwist(int(i) + 1), mgr.getTargetAcceleration(int(i) + 1)
        assert ok1 and ok2 and ok3
        got[j] = np.concatenate([pose, twist, acc])
    mgr.close()
    rows = Rows(dtype)
    rows.hold("init + getTargetPose", m, "now", got, same["now"][sel], sel, pose_only=True)
    assert (got[:, 7:] == 0).all()       # zero rates and accelerations in, exact zeros out (EarBase times zero rates too)
    rows.done(5)


# ---- pose streams of three predict-only ticks ---------------------------------------------------------------------------------
def _zeros(b, ld):
    """measurements nobody has: [3, 7, ld] of zeros in the batch's precision, has_meas [3, ld] of zeros"""
    return (torch.zeros((TICKS, 7, ld), dtype=b.torch_dtype(), device="cuda"), torch.zeros((TICKS, ld), dtype=torch.uint8, device="cuda"))


def _stream(ld):
    return torch.full((TICKS, 7, ld), float("nan"), dtype=torch.float64, device="cuda")


def _ticks_of(buf, n):
    h = buf.cpu().numpy()
    assert np.isnan(h[:, :, n:]).all(), "a column beyond the batch size was written"
    return h[:, :, :n].transpose(0, 2, 1)


def _hold_ticks(rows, path, m, got, same, mgr, ids):
    """[3, M, 7] against the after-k-ticks rows; then the getter's pose equals the last tick bit for bit"""
    for k in range(TICKS):
        rows.hold("%s tick %d" % (path, k + 1), m, ("ticks", k), got[k], same["ticks"][k])
    p, _, _, found = mgr.get_est_batch(ids)
    assert found.all()
    np.testing.assert_array_equal(p, got[TICKS - 1], err_msg="%s: get_est_batch after the ticks is not the stream's last tick" % path)


@pytest.mark.parametrize("form", ["eager", "graph", "fused"])
@pytest.mark.parametrize("name,dtype,layout", [(n, d, l) for n in ak.ANGULAR for d in ("f64", "f32") for l in ("auto", "201", "packed")])
def test_pose_streams_of_a_batch(models, name, dtype, layout, form):
    """poses= of Batch.step_sequence (eager and recorded) and of Batch.step_fused: the separable layouts write from the step
    kernel's POSE variant, the dense ones through the pose writer."""
    mm = ak.Model(name)
    m, mgr, b, ids = _manager(models, name, dtype, layout, cases=mm.tick_cases)
    same = ak.oracle_outputs(oracle, models, name, dtype)
    n = b.size
    meas, has = _zeros(b, n + 7)
    buf = _stream(n + 7)
    if form == "fused":
        b.step_fused(m.dt, meas, has, poses=buf)
    else:
        b.step_sequence(m.dt, meas, has, use_graph=(form == "graph"), poses=buf)
    torch.cuda.synchronize()
    rows = Rows(dtype)
    _hold_ticks(rows, "%s poses= %s" % ("step_fused" if form == "fused" else "step_sequence " + form, layout), m, _ticks_of(buf, n), same, mgr, ids)
    mgr.close()
    rows.done(TICKS)


@pytest.mark.parametrize("form", ["step_sequence_all", "step_fused_all"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pose_streams_of_a_manager_with_both_angular_models(models, dtype, form):
    """the population tick (one launch per tick for both batches) and the temporally fused replay of the manager"""
    mgr = te.TargetManager(dtype=dtype)
    parts, base = [], 0
    for name in ak.ANGULAR:
        m, mod = ak.Model(name), models[name]
        p0, v0, a0 = m.inputs(cases=m.tick_cases)
        ids = np.arange(len(p0), dtype=np.uint32) + base
        base += len(p0)
        assert mgr.init_batch(ids, m.dt, 0.0, p0, v0, a0, type=te.MODEL_TYPES[name], Q=mod["Q"], R=mod["R"], P0=mod["P"]) == len(p0)
        parts.append((m, ids))
    bs = mgr.batches()
    assert len(bs) == 2 and [b.size for b in bs] == [len(i) for _, i in parts]
    assert mgr.population_tick()
    zs = [_zeros(b, b.size + 3) for b in bs]
    bufs = [_stream(b.size + 3) for b in bs]
    if form == "step_sequence_all":
        mgr.step_sequence_all(parts[0][0].dt, [z[0] for z in zs], has_meas=[z[1] for z in zs], use_graph=0, poses=bufs)
    else:
        mgr.step_fused_all(parts[0][0].dt, [z[0] for z in zs], has_meas=[z[1] for z in zs], poses=bufs)
    torch.cuda.synchronize()
    rows = Rows(dtype)
    for (m, ids), b, buf in zip(parts, bs, bufs):
        _hold_ticks(rows, "%s poses=" % form, m, _ticks_of(buf, b.size), ak.oracle_outputs(oracle, models, m.name, dtype), mgr, ids)
    mgr.close()
    rows.done(2 * TICKS)


@pytest.mark.parametrize("name,dtype", [(n, d) for n in ak.ANGULAR for d in ("f64", "f32")])
def test_pose_output_of_a_resident_session(models, name, dtype):
    """live_set_pose_output: the ticks posted one at a time, the buffer copied on a second stream after each (the session, its
    posts and its stop as in tests/test_gpu_live.py)."""
    m = ak.Model(name)
    same = ak.oracle_outputs(oracle, models, name, dtype)
    p0, v0, a0 = m.inputs(cases=m.tick_cases)
    n = len(p0)
    ids = _ids(n)
    live = torch.cuda.Stream()
    mgr = te.TargetManager(model_path(name), dtype=dtype)
    mgr.set_stream(live.cuda_stream)
    assert mgr.init_batch(ids, m.dt, 0.0, p0, v0, a0) == n
    mgr.synchronize()
    b = mgr.batches()[0]
    ld = n + 13
    meas, has = _zeros(b, ld)
    pose_soa = torch.full((7, ld), float("nan"), dtype=torch.float64, device="cuda")
    host = torch.empty((7, ld), dtype=torch.float64).pin_memory()
    torch.cuda.synchronize()
    copy = torch.cuda.Stream()
    b.live_set_pose_output(pose_soa)
    b.live_start(m.dt, meas, has, max_ticks=TICKS, idle_limit_s=3.0)
    got = np.zeros((TICKS, n, 7))
    for s in range(TICKS):
        b.live_post(1)
        assert b.live_wait(s + 1, 5.0)
        with torch.cuda.stream(copy):
            host.copy_(pose_soa, non_blocking=True)
        copy.synchronize()
        got[s] = host.numpy()[:, :n].T
        assert np.isnan(host.numpy()[:, n:]).all()
    assert b.live_done() == TICKS and b.live_stop() == TICKS
    b.live_set_pose_output(None)
    rows = Rows(dtype)
    _hold_ticks(rows, "resident session pose output", m, got, same, mgr, ids)
    mgr.close()
    rows.done(TICKS)
