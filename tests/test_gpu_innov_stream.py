"""Per-tick innovation / NIS streams from launched ticks (target_batch_step_sequence_innov,
target_manager_step_sequence_all_innov): after every tick the innovation nu = y - x^-[0:m] and NIS = nu^T S^-1 nu of every target,
-1 and zeros where it had no measurement.

The reference of every numeric check is np_twin.Target, one per target, and the bound is derived from TOL[dtype] of
tests/test_gpu_parity.py (tests/innov_stream_ref.py); every target of every tick is compared.  "Bit-equal" compares two runs of
the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import innov_stream_ref as ref
import oracle
from conftest import HARNESS_ORDER, model_path, synth_stream
from test_gpu_parity import LANES, TOL, coupled

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

TICKS, DT, N0, SEED = 20, 0.004, 203, 31
NAN = float("nan")


def _soa(meas, dtype, ld):
    """meas [ticks,N,7] numpy -> CUDA SoA tensor [ticks,7,ld] in the precision"""
    tdt = torch.float64 if dtype == "f64" else torch.float32
    soa = torch.zeros((meas.shape[0], 7, ld), dtype=tdt, device="cuda")
    soa[:, :, :meas.shape[1]] = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).to("cuda").to(tdt)
    return soa


def _inputs(name, dtype, N, ticks, seed, ld):
    """the shared stream and twin reference of (name, N, ticks, seed) with its CUDA tensors: p0, soa, mask (numpy), has (CUDA), want"""
    p0, meas, mask, want = ref.stream_and_reference(name, N, ticks, seed)
    return p0, meas, _soa(meas, dtype, ld), mask, torch.from_numpy(mask.copy()).cuda(), want


def _bufs(blocks, m, ld, nu=True):
    nis = torch.full((blocks, ld), NAN, dtype=torch.float64, device="cuda")
    return nis, (torch.full((blocks, m, ld), NAN, dtype=torch.float64, device="cuda") if nu else None)


def _read(bufs, N):
    """(nis [blocks,N], nu [blocks,N,m] or None) numpy; the padding beyond N must still be NaN"""
    torch.cuda.synchronize()
    nis = bufs[0].cpu().numpy()
    assert np.isnan(nis[:, N:]).all(), "a NIS column beyond the batch size was written"
    nu = None
    if bufs[1] is not None:
        nu = bufs[1].cpu().numpy()
        assert np.isnan(nu[:, :, N:]).all(), "an innovation column beyond the batch size was written"
        nu = nu[:, :, :N].transpose(0, 2, 1)
    return nis[:, :N], nu


def _manager(name, dtype, lanes=0, classes=None, QRP=None, **kw):
    if classes is not None or QRP is not None:
        return te.TargetManager(dtype=dtype, **kw)
    return te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=lanes, **kw)


def _init(mgr, ids, p0, classes=None, QRP=None):
    if classes is not None:
        Q, R, P0, class_of, model = classes
        assert mgr.init_batch_classes(ids, DT, 0.0, p0, model, Q, R, P0, class_of) == len(ids)
    elif QRP is not None:
        Q, R, P0, model = QRP
        assert mgr.init_batch(ids, DT, 0.0, p0, type=model, Q=Q, R=R, P0=P0) == len(ids)
    else:
        assert mgr.init_batch(ids, DT, 0.0, p0) == len(ids)


def _m_of(name):
    return 6 if name.startswith("angular") else 3


CASES = [(m, d, g) for m in HARNESS_ORDER for d in ("f64", "f32") for g in LANES[m][d]]


@pytest.mark.parametrize("name,dtype,lanes", CASES)
def test_innovations_of_every_layout(name, dtype, lanes):
    """Test 1: every layout of LANES (0 / 201 / 301: the INNOV step kernels, in fp64 0 and 301 in the shared-axes form; every other
    code: the innovation writer ahead of the step), eager and recorded, 203 targets, 20 ticks with masks and a predict-only run: nu
    and NIS within the bound at every tick, sentinels exactly where the mask is 0, padding untouched, and the state the same bits as
    a manager stepped by the plain step_sequence."""
    N, ld, m = N0, N0 + 13, _m_of(name)
    p0, meas, soa, mask, has, want = _inputs(name, dtype, N, TICKS, SEED, ld)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    runs = {}
    for form in ("eager", "graph", "plain"):
        mgr = _manager(name, dtype, lanes)
        _init(mgr, ids, p0)
        b = mgr.batches()[0]
        bufs = _bufs(TICKS, m, ld)
        if form == "plain":
            b.step_sequence(DT, soa, has, use_graph=False)
        else:
            b.step_sequence(DT, soa, has, use_graph=form == "graph", innov=bufs)
            nis, nu = _read(bufs, N)
            ref.check(nu, nis, want, mask, dtype, "%s %s %d %s" % (name, dtype, lanes, form))
            runs[form + "_out"] = (nis, nu)
        torch.cuda.synchronize()
        runs[form] = mgr.get_state_batch(ids)
        mgr.close()
    for form in ("eager", "graph"):
        np.testing.assert_array_equal(runs[form][0], runs["plain"][0])
        np.testing.assert_array_equal(runs[form][1], runs["plain"][1])
    np.testing.assert_array_equal(runs["eager_out"][0], runs["graph_out"][0])
    np.testing.assert_array_equal(runs["eager_out"][1], runs["graph_out"][1])


@pytest.mark.parametrize("name,dtype,lanes", [("angular_velocities", "f64", 0), ("angular_rates", "f32", 301), ("uniform_acceleration", "f64", 201),
                                              ("uniform_velocity", "f64", 1), ("angular_velocities", "f32", 101)])
def test_nis_only_gives_the_same_nis(name, dtype, lanes):
    """Test 2: innov_dev NULL: the same NIS bits as with the innovation block (INNOV kernels and the writer)."""
    N, ld, m = N0, N0 + 13, _m_of(name)
    p0, meas, soa, mask, has, want = _inputs(name, dtype, N, TICKS, SEED, ld)
    ids = np.arange(N, dtype=np.uint32)
    got = []
    for with_nu in (True, False):
        mgr = _manager(name, dtype, lanes)
        _init(mgr, ids, p0)
        bufs = _bufs(TICKS, m, ld, nu=with_nu)
        mgr.batches()[0].step_sequence(DT, soa, has, innov=bufs)
        got.append(_read(bufs, N)[0])
        mgr.close()
    np.testing.assert_array_equal(got[0], got[1])
    ref.check(None, got[1], want, mask, dtype, "%s %s %d NIS only" % (name, dtype, lanes))


@pytest.mark.parametrize("use_graph", [False, True])
def test_ring_and_overwrite(use_graph):
    """Test 3: a ring of 3 blocks over 20 ticks holds ticks 18, 19, 17 (block s % 3); one block holds the last tick only."""
    name, dtype, N, m = "angular_rates", "f64", N0, 6
    p0, meas, soa, mask, has, want = _inputs(name, dtype, N, TICKS, SEED, N)
    ids = np.arange(N, dtype=np.uint32)
    mgr = _manager(name, dtype)
    _init(mgr, ids, p0)
    full = _bufs(TICKS, m, N)
    mgr.batches()[0].step_sequence(DT, soa, has, innov=full)
    nis_all, nu_all = _read(full, N)
    mgr.close()
    for blocks in (3, 1):
        mgr = _manager(name, dtype)
        _init(mgr, ids, p0)
        bufs = _bufs(blocks, m, N)
        mgr.batches()[0].step_sequence(DT, soa, has, use_graph=use_graph, innov=bufs)
        nis, nu = _read(bufs, N)
        for k in range(blocks):
            s = max(s for s in range(TICKS) if s % blocks == k)
            np.testing.assert_array_equal(nis[k], nis_all[s])
            np.testing.assert_array_equal(nu[k], nu_all[s])
        mgr.close()


def _pop_manager(models, parts, dtype, ticks, seed):
    from target_estimation_amd.streams import make_stream
    mgr = te.TargetManager(dtype=dtype)
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    base, meas, ids = 0, [], []
    for k, (name, n) in enumerate(parts):
        m = models[name]
        st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, seed + 17 * k, dtype=dtype)
        i = np.arange(n, dtype=np.uint32) + base
        base += n
        assert mgr.init_batch(i, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
        meas.append(st["meas"])
        ids.append(i)
    return mgr, meas, ids


def _pop_masks(parts, ticks, seed):
    out = []
    for k, (_, n) in enumerate(parts):
        h = ref.masks(ticks, n, seed + k).copy()
        h[min(2, ticks - 1)] = 0    # (a tick nobody is measured on, whatever the length)
        out.append(torch.from_numpy(h).cuda())
    return out


POP = [([("angular_rates", 331), ("angular_velocities", 203)], "f64", True), ([("angular_rates", 331), ("angular_velocities", 203)], "f32", False),
       ([("uniform_velocity", 203), ("uniform_acceleration", 130)], "f64", None)]


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("parts,dtype,shared", POP)
def test_population_tick(models, parts, dtype, shared, use_graph):
    """Test 4: the one-launch population tick with one stream per batch (the second batch NIS only), eager and recorded: the streams
    bit-equal to per-batch step_sequence_innov calls, the states bit-equal to a run without streams."""
    ticks = 6
    has = _pop_masks(parts, ticks, 5)
    # per-batch calls
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 77)
    want = []
    for i, b in enumerate(mgr.batches()):
        bufs = _bufs(ticks, b.meas_dim, b.size + 5, nu=i == 0)
        b.step_sequence(DT, meas[i], has[i], innov=bufs)
        want.append(_read(bufs, b.size))
    mgr.close()
    # without streams
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 77)
    mgr.step_sequence_all(DT, meas, has_meas=has, use_graph=use_graph)
    torch.cuda.synchronize()
    plain = [mgr.get_state_batch(i) for i in ids]
    mgr.close()
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 77)
    assert mgr.population_tick()
    bs = mgr.batches()
    if shared is not None:
        assert [b.shared_axes for b in bs] == [1 if shared else 0] * len(bs)
    bufs = [_bufs(ticks, b.meas_dim, b.size + 5, nu=i == 0) for i, b in enumerate(bs)]
    mgr.step_sequence_all(DT, meas, has_meas=has, use_graph=use_graph, innov=bufs)
    assert mgr.population_tick()
    for i, b in enumerate(bs):
        nis, nu = _read(bufs[i], b.size)
        np.testing.assert_array_equal(nis, want[i][0])
        if i == 0:
            np.testing.assert_array_equal(nu, want[i][1])
        assert (nis[2] == -1.0).all() and (nis[0] >= 0).any()
        x, P = mgr.get_state_batch(ids[i])
        np.testing.assert_array_equal(x, plain[i][0])
        np.testing.assert_array_equal(P, plain[i][1])
    if shared is not None:
        assert [b.shared_axes for b in bs] == [1 if shared else 0] * len(bs)
    # one batch with a stream, the other without: the other's buffers stay untouched
    mgr.close()
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 77)
    bs = mgr.batches()
    only = _bufs(ticks, bs[1].meas_dim, bs[1].size + 5, nu=False)
    mgr.step_sequence_all(DT, meas, has_meas=has, use_graph=use_graph, innov=[None, only])
    np.testing.assert_array_equal(_read(only, bs[1].size)[0], want[1][0])
    mgr.close()


@pytest.mark.parametrize("name", ["uniform_velocity", "angular_rates", "angular_velocities"])
def test_shared_form_and_uniform_tiles(models, name):
    """Test 5: 130 fp64 targets in the shared-axes form (uniform tiles where the model has them): four all-measured dense ticks, one
    tick whose mask splits tile 0, two more.  The batch stays in the form, its uniform tiles are those of a twin manager without
    a stream after every phase, the states are the same bits, and nu / NIS are within the bound throughout."""
    dtype, N, m, ticks = "f64", 130, _m_of(name), 7
    mdl = models[name]
    p0, meas, _, _ = ref.stream_and_reference(name, N, ticks, 9)
    p0 = np.tile(p0[:1], (N, 1))     # (the covariance words do not depend on it; the positions do)
    mask = np.ones((ticks, N), np.uint8)
    mask[4, 5:40] = 0
    want = ref.twin_innovations(mdl["model"], mdl["Q"], mdl["R"], mdl["P"], p0, meas, mask, DT)
    soa, has = _soa(meas, dtype, N), torch.from_numpy(mask).cuda()
    ids = np.arange(N, dtype=np.uint32)
    a, t = _manager(name, dtype), _manager(name, dtype)
    _init(a, ids, p0)
    _init(t, ids, p0)
    ab, tb = a.batches()[0], t.batches()[0]
    bufs = _bufs(ticks, m, N)
    seen = []
    for lo, hi, masked in ((0, 4, False), (4, 5, True), (5, 7, False)):
        sub = (bufs[0][lo:hi], bufs[1][lo:hi])
        ab.step_sequence(DT, soa[lo:hi], has[lo:hi] if masked else None, innov=sub)
        tb.step_sequence(DT, soa[lo:hi], has[lo:hi] if masked else None)
        torch.cuda.synchronize()
        assert ab.shared_axes == 1 and tb.shared_axes == 1
        assert ab.uniform_tiles == tb.uniform_tiles
        seen.append(ab.uniform_tiles)
    if name != "angular_velocities":
        assert seen[0] > 0, "no tile became uniform: the test does not reach the uniform-tile path"
    xa, Pa = a.get_state_batch(ids)
    xt, Pt = t.get_state_batch(ids)
    np.testing.assert_array_equal(xa, xt)
    np.testing.assert_array_equal(Pa, Pt)
    nis, nu = _read(bufs, N)
    ref.check(nu, nis, want, mask, dtype, "%s shared form" % name)
    a.close()
    t.close()


def _ab_zigzag_scenario():
    """innovation streams and final states, with and without the stream, of an eager sequence on a separable fp64 batch and a
    separable fp32 batch (INNOV kernels), a coupled-matrix batch (the writer) and a two-model population tick"""
    from conftest import MODEL_FILES
    models = {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}
    out = {}
    ticks = 7
    for key, (name, dtype, QRP) in {"sep_f64": ("angular_rates", "f64", False), "sep_f32": ("uniform_acceleration", "f32", False),
                                    "dense": ("angular_velocities", "f64", True)}.items():
        N = 331
        p0, meas, mask, _ = ref.stream_and_reference(name, N, ticks, 3)
        soa, has = _soa(meas, dtype, N), torch.from_numpy(mask.copy()).cuda()
        ids = np.arange(N, dtype=np.uint32)
        kw = {}
        if QRP:
            c = coupled(models[name])
            kw = dict(QRP=(c["Q"], c["R"], c["P"], models[name]["model"]))
        for with_stream in (True, False):
            mgr = _manager(name, dtype, **kw)
            _init(mgr, ids, p0, **kw)
            bufs = _bufs(ticks, _m_of(name), N)
            mgr.batches()[0].step_sequence(DT, soa, has, innov=bufs if with_stream else None)
            torch.cuda.synchronize()
            x, P = mgr.get_state_batch(ids)
            tag = key + ("" if with_stream else "_plain")
            out[tag + "_x"], out[tag + "_P"] = x, P
            if with_stream:
                out[key + "_nis"], out[key + "_nu"] = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
            mgr.close()
    parts = [("angular_rates", 900), ("uniform_velocity", 800)]
    for with_stream in (True, False):
        mgr, meas, ids = _pop_manager(models, parts, "f64", ticks, 11)
        bufs = [_bufs(ticks, b.meas_dim, b.size) for b in mgr.batches()]
        mgr.step_sequence_all(DT, meas, use_graph=0, innov=bufs if with_stream else None)
        torch.cuda.synchronize()
        for i in range(2):
            x, P = mgr.get_state_batch(ids[i])
            tag = "pop%d" % i + ("" if with_stream else "_plain")
            out[tag + "_x"], out[tag + "_P"] = x, P
            if with_stream:
                out["pop%d_nis" % i], out["pop%d_nu" % i] = bufs[i][0].cpu().numpy(), bufs[i][1].cpu().numpy()
        mgr.close()
    return out


def _ab_zigzag_child(path):
    np.savez(path, **_ab_zigzag_scenario())
    print("innovation scenario ok")


@pytest.mark.parametrize("env", ["TE_PINGPONG_MIN_MB", "TE_ZIGZAG_MIN_MB"])
def test_forced_ab_and_zigzag_ticks(tmp_path, env):
    """Test 6: a child process in which every eager tick without a stream is an A -> B tick (TE_PINGPONG_MIN_MB=0), one in which
    every tick zig-zags (TE_ZIGZAG_MIN_MB=0): the streams equal those of in-place, forward ticks in this process bit for bit, and
    in both processes the state behind a call with a stream equals the state behind the call without one."""
    path = str(tmp_path / "innov.npz")
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    e[env] = "0"
    p = subprocess.run([sys.executable, "-c", "import test_gpu_innov_stream as t; t._ab_zigzag_child(%r)" % path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "innovation scenario ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    child = np.load(path)
    here = _ab_zigzag_scenario()
    for k, v in here.items():
        np.testing.assert_array_equal(child[k], v, err_msg=k)
        assert not np.isnan(v).any(), k
    for res in (child, here):
        for key in ("sep_f64", "sep_f32", "dense", "pop0", "pop1"):
            np.testing.assert_array_equal(res[key + "_x"], res[key + "_plain_x"], err_msg=key)
            np.testing.assert_array_equal(res[key + "_P"], res[key + "_plain_P"], err_msg=key)


@pytest.mark.parametrize("name,dtype,lanes", [("angular_velocities", "f64", 0), ("uniform_acceleration", "f32", 301), ("angular_rates", "f64", 6)])
def test_with_poses_in_the_same_call(name, dtype, lanes):
    """Test 7a: poses and innovations in one call: the poses bit-equal to the _poses call, the innovations to the call without poses."""
    N, ld, m = N0, N0 + 13, _m_of(name)
    p0, meas, soa, mask, has, want = _inputs(name, dtype, N, TICKS, SEED, ld)
    ids = np.arange(N, dtype=np.uint32)
    res = {}
    for form in ("both", "poses", "innov"):
        for use_graph in (False, True):
            mgr = _manager(name, dtype, lanes)
            _init(mgr, ids, p0)
            poses = torch.full((TICKS, 7, ld), NAN, dtype=torch.float64, device="cuda")
            bufs = _bufs(TICKS, m, ld)
            mgr.batches()[0].step_sequence(DT, soa, has, use_graph=use_graph, poses=poses if form != "innov" else None,
                                           innov=bufs if form != "poses" else None)
            torch.cuda.synchronize()
            res[form, use_graph] = (poses.cpu().numpy(), bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), mgr.get_state_batch(ids))
            mgr.close()
    for g in (False, True):
        np.testing.assert_array_equal(res["both", g][0], res["poses", False][0])
        np.testing.assert_array_equal(res["both", g][1], res["innov", False][1])
        np.testing.assert_array_equal(res["both", g][2], res["innov", False][2])
        np.testing.assert_array_equal(res["both", g][3][0], res["poses", False][3][0])
        np.testing.assert_array_equal(res["both", g][3][1], res["poses", False][3][1])
    assert not np.isnan(res["both", False][0][:, :, :N]).any() and not np.isnan(res["both", False][1][:, :N]).any()


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("parts", [[("angular_rates", 331), ("angular_velocities", 203)], [("uniform_acceleration", 203)]])
def test_with_query_and_poses_at_the_manager(models, parts, use_graph):
    """Test 7b: step_sequence_all with the fused query, pose streams and innovation streams together (a population tick, and a
    manager with one batch): poses and query results bit-equal to the _poses call, innovations bit-equal to the call without them."""
    dtype, ticks = "f64", 5
    origin, radius = np.array([0.5, -0.25, 0.1]), 6.0
    has = _pop_masks(parts, ticks, 8)
    res = {}
    for form in ("all", "poses", "innov"):
        mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 77)
        bs = mgr.batches()
        poses = [torch.full((ticks, 7, b.size + 3), NAN, dtype=torch.float64, device="cuda") for b in bs]
        bufs = [_bufs(ticks, b.meas_dim, b.size + 3) for b in bs]
        deltas = [torch.full((b.size,), NAN, dtype=torch.float64, device="cuda") for b in bs]
        qposes = [torch.full((b.size, 7), NAN, dtype=torch.float64, device="cuda") for b in bs]
        mgr.step_sequence_all(DT, meas, has_meas=has, query=None if form == "innov" else (origin, radius, deltas, qposes), use_graph=use_graph,
                              poses=None if form == "innov" else poses, innov=None if form == "poses" else bufs)
        torch.cuda.synchronize()
        res[form] = dict(poses=[p.cpu().numpy() for p in poses], nis=[b[0].cpu().numpy() for b in bufs], nu=[b[1].cpu().numpy() for b in bufs],
                         delta=[d.cpu().numpy() for d in deltas], qpose=[q.cpu().numpy() for q in qposes],
                         state=[mgr.get_state_batch(i) for i in ids])
        mgr.close()
    for i in range(len(parts)):
        for k in ("poses", "delta", "qpose"):
            np.testing.assert_array_equal(res["all"][k][i], res["poses"][k][i], err_msg=k)
            assert not np.isnan(res["all"][k][i][..., :parts[i][1]] if k == "poses" else res["all"][k][i]).any()
        for k in ("nis", "nu"):
            np.testing.assert_array_equal(res["all"][k][i], res["innov"][k][i], err_msg=k)
        for j in (0, 1):
            np.testing.assert_array_equal(res["all"]["state"][i][j], res["poses"]["state"][i][j])


_FALLBACK_REF = {}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["coupled", "classes"])
def test_fallback_layouts(models, kind, dtype):
    """Test 8: a coupled-matrix batch (the dense kernel) and a 3-class batch (the per-class kernels): the innovation writer ahead of
    each step, within the bound against one twin per class, eager and recorded; the state as without a stream."""
    name, N, m = "angular_rates", 131, 6
    mdl = models[name]
    p0, meas, mask, _ = ref.stream_and_reference(name, N, TICKS, 21)
    soa, has = _soa(meas, dtype, N + 3), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    if kind == "coupled":
        c = coupled(mdl)
        kw = dict(QRP=(c["Q"], c["R"], c["P"], mdl["model"]))
        if kind not in _FALLBACK_REF:   # (one twin run for both precisions)
            _FALLBACK_REF[kind] = ref.twin_innovations(mdl["model"], c["Q"], c["R"], c["P"], p0, meas, mask, DT)
        want = _FALLBACK_REF[kind]
    else:
        scale = np.array([1.0, 2.0, 0.5])
        Q = np.stack([mdl["Q"] * s for s in scale]); R = np.stack([mdl["R"] * s for s in scale]); P0 = np.stack([mdl["P"]] * 3)
        class_of = (np.arange(N) % 3).astype(np.uint32)
        kw = dict(classes=(Q, R, P0, class_of, mdl["model"]))
        want = _FALLBACK_REF.get(kind)
        for k in range(3 if want is None else 0):
            sel = class_of == k
            w = ref.twin_innovations(mdl["model"], Q[k], R[k], P0[k], p0[sel], meas[:, sel], mask[:, sel], DT)
            if want is None:
                want = {key: np.zeros(v.shape[:1] + (N,) + v.shape[2:]) for key, v in w.items() if key not in ("x", "P")}
            for key in want:
                want[key][:, sel] = w[key]
        _FALLBACK_REF[kind] = want
    states = []
    for form in ("eager", "graph", "plain"):
        mgr = _manager(name, dtype, **kw)
        _init(mgr, ids, p0, **kw)
        b = mgr.batches()[0]
        if kind == "coupled":
            assert b.layout in ("full", "symmetric_packed")
        else:
            assert b.num_classes == 3
        bufs = _bufs(TICKS, m, N + 3)
        b.step_sequence(DT, soa, has, use_graph=form == "graph", innov=None if form == "plain" else bufs)
        if form != "plain":
            nis, nu = _read(bufs, N)
            ref.check(nu, nis, want, mask, dtype, "%s %s %s" % (kind, dtype, form))
        torch.cuda.synchronize()
        states.append(mgr.get_state_batch(ids))
        mgr.close()
    for s in states[:2]:
        np.testing.assert_array_equal(s[0], states[2][0])
        np.testing.assert_array_equal(s[1], states[2][1])


def test_several_classes_with_poses_in_the_same_call(models):
    """Test 8b: a 3-class batch of the separable layout with a pose stream AND an innovation stream in one eager call -- the
    innovation writer ahead of each per-class step, the pose writer behind it.  65 targets (a wavefront and one lane), 3 ticks,
    target 7 without a measurement on tick 2: every tick's innovations within test 8's bound against one twin per class, every
    tick's poses within the pose stream's output tolerance against the oracle, the state as without the streams."""
    name, dtype, N, ticks, m = "angular_rates", "f64", 65, 3, 6
    mdl = models[name]
    p0, meas = synth_stream(name, N, ticks, seed=23)
    mask = np.ones((ticks, N), np.uint8)
    mask[1, 7] = 0
    soa, has = _soa(meas, dtype, N + 3), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    scale = np.array([1.0, 2.0, 0.5])
    Q = np.stack([mdl["Q"] * s for s in scale]); R = np.stack([mdl["R"] * s for s in scale]); P0 = np.stack([mdl["P"]] * 3)
    class_of = (np.arange(N) % 3).astype(np.uint32)
    kw = dict(classes=(Q, R, P0, class_of, mdl["model"]))
    want, want_pose = None, np.zeros((ticks, N, 7))
    for k in range(3):
        sel = class_of == k
        w = ref.twin_innovations(mdl["model"], Q[k], R[k], P0[k], p0[sel], meas[:, sel], mask[:, sel], DT)
        if want is None:
            want = {key: np.zeros(v.shape[:1] + (N,) + v.shape[2:]) for key, v in w.items() if key not in ("x", "P")}
        for key in want:
            want[key][:, sel] = w[key]
        orc = oracle.OracleBatch(mdl["model"], Q[k], R[k], P0[k], p0[sel], DT, dtype=dtype)
        for s in range(ticks):
            orc.step(DT, meas[s, sel], mask[s, sel])
            want_pose[s, sel] = orc.pose()
    states = []
    for form in ("both", "plain"):
        mgr = _manager(name, dtype, **kw)
        _init(mgr, ids, p0, **kw)
        b = mgr.batches()[0]
        assert b.num_classes == 3 and b.layout.startswith("axis_separable")
        poses = torch.full((ticks, 7, N + 3), NAN, dtype=torch.float64, device="cuda")
        bufs = _bufs(ticks, m, N + 3)
        b.step_sequence(DT, soa, has, use_graph=False, poses=poses if form == "both" else None, innov=bufs if form == "both" else None)
        if form == "both":
            nis, nu = _read(bufs, N)
            ref.check(nu, nis, want, mask, dtype, "3 classes with poses")
            h = poses.cpu().numpy()
            assert np.isnan(h[:, :, N:]).all(), "a pose column beyond the batch size was written"
            got = h[:, :, :N].transpose(0, 2, 1)
            print("worst pose error %.3g (tolerance %.3g)" % (np.abs(got - want_pose).max(), TOL[dtype]["out_atol"]))
            np.testing.assert_allclose(got, want_pose, atol=TOL[dtype]["out_atol"], rtol=0)
        torch.cuda.synchronize()
        states.append(mgr.get_state_batch(ids))
        mgr.close()
    np.testing.assert_array_equal(states[0][0], states[1][0])
    np.testing.assert_array_equal(states[0][1], states[1][1])


def test_columns_follow_slot_ids_after_erase():
    """Test 9: after a third of the targets is erased, column j is the innovation of target slot_ids()[j]: the bits a manager that
    erased nothing writes in that target's column."""
    name, dtype, N, ticks, m = "angular_velocities", "f64", 300, 3, 6
    p0, meas, mask, _ = ref.stream_and_reference(name, N, ticks, 13)
    soa, has = _soa(meas, dtype, N), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32) + 1000
    out = []
    for erase in (False, True):
        mgr = _manager(name, dtype)
        _init(mgr, ids, p0)
        b = mgr.batches()[0]
        b.step(DT, soa[0])
        cols = np.arange(N)
        meas_k, has_k = soa[1:], has[1:]
        if erase:
            assert mgr.erase_batch(ids[::3]) == len(ids[::3])
            slot_ids = b.slot_ids()
            assert b.size == N - len(ids[::3]) and not np.isin(slot_ids, ids[::3]).any()
            cols = (slot_ids - 1000).astype(np.int64)
            idx = torch.from_numpy(cols).cuda()
            meas_k = torch.zeros_like(soa[1:])
            meas_k[:, :, :b.size] = soa[1:][:, :, idx]
            has_k = torch.zeros_like(has[1:])
            has_k[:, :b.size] = has[1:][:, idx]
        bufs = _bufs(ticks - 1, m, N)
        b.step_sequence(DT, meas_k, has_k, innov=bufs)
        out.append((_read(bufs, b.size), cols))
        mgr.close()
    (nis_all, nu_all), _ = out[0]
    (nis_e, nu_e), cols = out[1]
    assert len(cols) == 200 and (cols != np.arange(200)).any()
    np.testing.assert_array_equal(nis_e, nis_all[:, cols])
    np.testing.assert_array_equal(nu_e, nu_all[:, cols])


def test_bad_innovation_streams_are_refused_and_launch_nothing(models):
    """Test 10: ld < size, a stride in (0, ld) / (0, m ld), negative values and ring_ticks < 0 return < 0 with an error message;
    state and buffers are untouched.  The manager-level call checks every batch's stream before it enqueues anything."""
    import ctypes as C
    from target_estimation_amd import capi
    lib = capi.lib()
    name, dtype, N, m = "angular_rates", "f64", 100, 6
    p0, meas, mask, _ = ref.stream_and_reference(name, N, 2, 4)
    soa = _soa(meas, dtype, N)
    ids = np.arange(N, dtype=np.uint32)
    mgr = _manager(name, dtype)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    x0, P0 = mgr.get_state_batch(ids)
    nis, nu = _bufs(2, m, N)
    bad = [(N - 1, N, m * N, 0), (N, N - 1, m * N, 0), (N, 1, m * N, 0), (N, N, m * N - 1, 0), (N, N, 1, 0), (-N, N, m * N, 0),
           (N, -N, m * N, 0), (N, N, -m * N, 0), (N, N, m * N, -1)]
    for ld, ns, us, ring in bad:
        for nu_ptr in (nu.data_ptr(), None):
            s = capi.InnovStream(nis.data_ptr(), nu_ptr, ld, ns, us, ring)
            for use_graph in (0, 1):
                rc = lib.target_batch_step_sequence_innov(b._h, 2, DT, soa.data_ptr(), soa.stride(0), soa.stride(1), None, 0, 0, None,
                                                          C.byref(s), use_graph)
                assert rc < 0 and "innovation stream" in capi.last_error(), (ld, ns, us, ring)
    with pytest.raises(RuntimeError, match="innovation stream"):
        b.step_sequence(DT, soa, innov=_bufs(2, m, N - 1))
    torch.cuda.synchronize()
    x1, P1 = mgr.get_state_batch(ids)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(P1, P0)
    assert torch.isnan(nis).all() and torch.isnan(nu).all()
    mgr.close()
    mgr, meas2, ids2 = _pop_manager(models, [("angular_rates", 300), ("uniform_velocity", 200)], "f64", 2, 3)
    xs = [mgr.get_state_batch(i) for i in ids2]
    good = _bufs(2, 6, 300)
    specs = (capi.BatchSequence * 2)()
    for i, t in enumerate(meas2):
        specs[i].meas_dev, specs[i].tick_stride, specs[i].ld = t.data_ptr(), t.stride(0), t.stride(1)
    small = _bufs(2, 3, 200)
    streams = (capi.InnovStream * 2)(capi.InnovStream(good[0].data_ptr(), good[1].data_ptr(), 300, 300, 6 * 300, 0),
                                     capi.InnovStream(small[0].data_ptr(), small[1].data_ptr(), 150, 150, 3 * 150, 0))   # ld 150 < 200
    for use_graph in (0, 1):
        rc = lib.target_manager_step_sequence_all_innov(mgr._h, 2, DT, C.cast(specs, C.c_void_p), None, streams, 2, 0, None, 0.0, use_graph)
        assert rc < 0 and "innovation stream" in capi.last_error()
    torch.cuda.synchronize()
    for i, (x, P) in zip(ids2, xs):
        x1, P1 = mgr.get_state_batch(i)
        np.testing.assert_array_equal(x1, x)
        np.testing.assert_array_equal(P1, P)
    assert all(torch.isnan(t).all() for t in (*good, *small))
    mgr.close()


def test_recorded_graphs_keep_their_own_innovation_buffers():
    """A recorded graph is keyed by the innovation stream too: two recordings that differ only in their buffers are two graphs."""
    name, dtype, N, ticks, m = "uniform_velocity", "f64", 130, 4, 3
    p0, meas, mask, _ = ref.stream_and_reference(name, N, ticks, 9)
    soa, has = _soa(meas, dtype, N), torch.from_numpy(mask.copy()).cuda()
    mgr = _manager(name, dtype)
    _init(mgr, np.arange(N, dtype=np.uint32), p0)
    b = mgr.batches()[0]
    A, B = _bufs(ticks, m, N), _bufs(ticks, m, N)
    b.step_sequence(DT, soa, has, use_graph=True, innov=A)
    torch.cuda.synchronize()
    a1 = (A[0].clone(), A[1].clone())
    b.step_sequence(DT, soa, has, use_graph=True, innov=B)
    torch.cuda.synchronize()
    assert torch.equal(A[0], a1[0]) and torch.equal(A[1], a1[1]), "the second graph wrote into the first one's buffers"
    assert not torch.isnan(B[0]).any() and not torch.equal(B[0], A[0])
    mgr.close()
