"""Per-tick pose streams from launched ticks (target_batch_step_sequence_poses, target_batch_step_fused_poses,
target_manager_step_sequence_all_poses): after every tick the estimated pose of every target, as the reference's node publishes it
(src/target_manager_ros.cpp:78-87).

"Bit-equal" compares with a twin manager stepped one target_batch_step per tick and read with target_batch_get_est_dev after each;
"oracle" holds the poses to the f64 / f32 output tolerance of tests/test_gpu_parity.py against the CPU oracle's pose()."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import HARNESS_ORDER, model_path, synth_stream
from test_gpu_parity import LANES, TOL, check_state, coupled

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

TICKS, DT = 20, 0.004
PREDICT_ONLY = range(11, 15)    # a run of ticks on which no target has a measurement
ORACLE_TICKS = (0, 9, 19)       # ticks 1, 10 and 20


def _inputs(name, dtype, N, ticks, seed, ld):
    """p0 [N,7]; meas [ticks,N,7] (numpy); the same as a CUDA SoA tensor [ticks,7,ld] in the precision; Bernoulli(0.9) masks with a
    predict-only run, numpy [ticks,N] and CUDA [ticks,N] uint8."""
    p0, meas = synth_stream(name, N, ticks, seed=seed)
    rng = np.random.default_rng(seed + 1)
    mask = (rng.random((ticks, N)) < 0.9).astype(np.uint8)
    for s in PREDICT_ONLY:
        if s < ticks:
            mask[s] = 0
    tdt = torch.float64 if dtype == "f64" else torch.float32
    soa = torch.zeros((ticks, 7, ld), dtype=tdt, device="cuda")
    soa[:, :, :N] = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).to("cuda").to(tdt)
    return p0, meas, soa, mask, torch.from_numpy(mask).cuda()


def _twin_poses(path, dtype, lanes, ids, p0, soa, has, dt=DT, **kw):
    """[ticks, N, 7]: a manager stepped one target_batch_step per tick, poses read with target_batch_get_est_dev after each."""
    mgr = _manager(path, dtype, lanes, kw)
    _init(mgr, ids, p0, **kw)
    b = mgr.batches()[0]
    out = []
    for s in range(soa.shape[0]):
        b.step(dt, soa[s], None if has is None else has[s])
        out.append(b.get_est(twist=False, acc=False)[0].cpu().numpy())
    x, P = mgr.get_state_batch(ids)
    mgr.close()
    return np.stack(out), x, P


def _manager(path, dtype, lanes, kw):
    """a manager of the model file, or (explicit matrices / classes) one that takes its batches from init_batch"""
    if kw.get("classes") is not None or kw.get("QRP") is not None:
        return te.TargetManager(dtype=dtype)
    return te.TargetManager(path, dtype=dtype, lanes_per_target=lanes)


def _init(mgr, ids, p0, classes=None, QRP=None):
    if classes is not None:
        Q, R, P0, class_of, model = classes
        assert mgr.init_batch_classes(ids, DT, 0.0, p0, model, Q, R, P0, class_of) == len(ids)
    elif QRP is not None:
        Q, R, P0, model = QRP
        assert mgr.init_batch(ids, DT, 0.0, p0, type=model, Q=Q, R=R, P0=P0) == len(ids)
    else:
        assert mgr.init_batch(ids, DT, 0.0, p0) == len(ids)


def _soa_poses(buf, N):
    """pose tensor [blocks, 7, ld] -> [blocks, N, 7] numpy; the padding beyond N must still be NaN"""
    h = buf.cpu().numpy()
    assert np.isnan(h[:, :, N:]).all(), "a column beyond the batch size was written"
    return h[:, :, :N].transpose(0, 2, 1)


def _oracle_poses(m, dtype, p0, meas, mask, ticks=ORACLE_TICKS, Q=None, R=None, P0=None):
    orc = oracle.OracleBatch(m["model"], m["Q"] if Q is None else Q, m["R"] if R is None else R, m["P"] if P0 is None else P0,
                             p0, DT, dtype=dtype)
    out = {}
    for s in range(meas.shape[0]):
        orc.step(DT, meas[s], mask[s])
        if s in ticks:
            out[s] = orc.pose()
    return out


def _check_oracle(got, want, dtype, what):
    for s, w in want.items():
        np.testing.assert_allclose(got[s], w, atol=TOL[dtype]["out_atol"], err_msg="%s, tick %d" % (what, s + 1))


CASES = [(m, d, g) for m in HARNESS_ORDER for d in ("f64", "f32") for g in LANES[m][d]]


@pytest.mark.parametrize("name,dtype,lanes", CASES)
def test_pose_stream_of_step_sequence_and_step_fused(models, name, dtype, lanes):
    """Cases 1-3: every layout (the separable ones 0 / 201 / 301 write from the step kernel, the dense ones through the pose
    writer), eager and recorded step_sequence_poses and step_fused_poses, 20 ticks with masks and a predict-only run: every tick's
    block bit-equal to the twin, within the oracle's tolerance at ticks 1, 10, 20, padding untouched, and the state records the
    same bits as a run without poses."""
    m = models[name]
    N = 203
    ld = N + 13
    path = model_path(name)
    p0, meas, soa, mask, has = _inputs(name, dtype, N, TICKS, 31, ld)
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    want, x_twin, P_twin = _twin_poses(path, dtype, lanes, ids, p0, soa, has)
    _check_oracle(want, _oracle_poses(m, dtype, p0, meas, mask), dtype, "%s %s %d twin" % (name, dtype, lanes))
    runs = {}
    for form in ("eager", "graph", "fused", "plain"):
        mgr = te.TargetManager(path, dtype=dtype, lanes_per_target=lanes)
        _init(mgr, ids, p0)
        b = mgr.batches()[0]
        poses = torch.full((TICKS, 7, ld), float("nan"), dtype=torch.float64, device="cuda")
        if form == "eager":
            b.step_sequence(DT, soa, has, use_graph=False, poses=poses)
        elif form == "graph":
            b.step_sequence(DT, soa, has, use_graph=True, poses=poses)
        elif form == "fused":
            b.step_fused(DT, soa, has, poses=poses)
        else:
            b.step_sequence(DT, soa, has, use_graph=False)
        torch.cuda.synchronize()
        runs[form] = mgr.get_state_batch(ids)
        if form != "plain":
            got = _soa_poses(poses, N)
            np.testing.assert_array_equal(got, want, err_msg="%s %s %d %s" % (name, dtype, lanes, form))
        mgr.close()
    for form in ("eager", "graph", "fused"):   # case 3: writing poses changes nothing else
        np.testing.assert_array_equal(runs[form][0], runs["plain"][0])
        np.testing.assert_array_equal(runs[form][1], runs["plain"][1])
    np.testing.assert_array_equal(runs["plain"][0], x_twin)
    np.testing.assert_array_equal(runs["plain"][1], P_twin)


@pytest.mark.parametrize("fused", [False, True])
def test_ring_and_overwrite(models, fused):
    """Case 4: a ring of 3 blocks over 10 ticks holds ticks 7-9 (block s % 3); tick_stride 0 holds the last tick only."""
    name, dtype, N, ticks = "angular_rates", "f64", 150, 10
    p0, meas, soa, mask, has = _inputs(name, dtype, N, ticks, 5, N)
    ids = np.arange(N, dtype=np.uint32)
    want, _, _ = _twin_poses(model_path(name), dtype, 0, ids, p0, soa, has)
    for blocks in (3, 1):
        mgr = te.TargetManager(model_path(name), dtype=dtype)
        _init(mgr, ids, p0)
        b = mgr.batches()[0]
        buf = torch.full((blocks, 7, N), float("nan"), dtype=torch.float64, device="cuda")
        if fused:
            b.step_fused(DT, soa, has, poses=buf)
        else:
            b.step_sequence(DT, soa, has, poses=buf)
        got = _soa_poses(buf, N)
        for k in range(blocks):
            s = max(s for s in range(ticks) if s % blocks == k)
            np.testing.assert_array_equal(got[k], want[s])
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


def _pop_twin(models, parts, dtype, ticks, seed, query=None):
    """per-batch launches: target_batch_step per batch per tick, get_est_dev (+ the own-time query) after each"""
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, seed)
    poses, q = [[] for _ in parts], None
    for s in range(ticks):
        for i, b in enumerate(mgr.batches()):
            b.step(DT, meas[i][s])
            poses[i].append(b.get_est(twist=False, acc=False)[0].cpu().numpy())
    if query is not None:
        q = [b.intersect_sphere(query[0], query[1]) for b in mgr.batches()]
        q = [(d.cpu().numpy(), p.cpu().numpy()) for d, p in q]
    torch.cuda.synchronize()
    mgr.close()
    return [np.stack(p) for p in poses], q


@pytest.mark.parametrize("use_graph", [0, 1])
def test_population_tick_with_poses_and_query(models, use_graph):
    """Case 5: configs[4]'s share (angular rates + angular velocities, fused own-time sphere query) as ONE launch per tick with
    the pose stream: poses and query results bit-equal to the per-batch launches; one batch's poses with the other's pose_dev NULL."""
    parts, dtype, ticks = [("angular_rates", 3001), ("angular_velocities", 2003)], "f64", 6
    origin, radius = np.array([0.5, -0.25, 0.1]), 6.0
    want, wq = _pop_twin(models, parts, dtype, ticks, 77, (origin, radius))
    for which in ("both", "first"):
        mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 77)
        assert mgr.population_tick()
        bs = mgr.batches()
        ld = [b.size + 5 for b in bs]
        bufs = [torch.full((ticks, 7, l), float("nan"), dtype=torch.float64, device="cuda") for l in ld]
        deltas = [torch.empty(b.size, dtype=torch.float64, device="cuda") for b in bs]
        qposes = [torch.empty((b.size, 7), dtype=torch.float64, device="cuda") for b in bs]
        poses = bufs if which == "both" else [bufs[0], None]
        mgr.step_sequence_all(DT, meas, query=(origin, radius, deltas, qposes), use_graph=use_graph, poses=poses)
        torch.cuda.synchronize()
        assert mgr.population_tick()
        for i, b in enumerate(bs):
            if poses[i] is None:
                assert torch.isnan(bufs[i]).all(), "a batch without a pose stream was written"
                continue
            np.testing.assert_array_equal(_soa_poses(bufs[i], b.size), want[i])
            np.testing.assert_array_equal(deltas[i].cpu().numpy(), wq[i][0])
            np.testing.assert_array_equal(qposes[i].cpu().numpy(), wq[i][1])
        mgr.close()


def _ab_zigzag_scenario():
    """poses of an eager sequence on a separable batch (the POSE kernel), a coupled-matrix batch (the pose writer) and a
    two-model population tick, as numpy arrays"""
    from conftest import MODEL_FILES
    models = {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}
    out = {}
    ticks = 7
    for key, (name, dtype, QRP) in {"sep_f64": ("angular_rates", "f64", False), "sep_f32": ("uniform_acceleration", "f32", False),
                                    "dense": ("angular_velocities", "f64", True)}.items():
        N = 700
        p0, meas, soa, mask, has = _inputs(name, dtype, N, ticks, 3, N)
        m = models[name]
        mgr = te.TargetManager(dtype=dtype) if QRP else te.TargetManager(model_path(name), dtype=dtype)
        if QRP:
            c = coupled(m)
            _init(mgr, np.arange(N, dtype=np.uint32), p0, QRP=(c["Q"], c["R"], c["P"], m["model"]))
        else:
            _init(mgr, np.arange(N, dtype=np.uint32), p0)
        buf = torch.full((ticks, 7, N), float("nan"), dtype=torch.float64, device="cuda")
        mgr.batches()[0].step_sequence(DT, soa, has, poses=buf)
        out[key] = buf.cpu().numpy()
        mgr.close()
    mgr, meas, ids = _pop_manager(models, [("angular_rates", 900), ("uniform_velocity", 800)], "f64", ticks, 11)
    bufs = [torch.full((ticks, 7, b.size), float("nan"), dtype=torch.float64, device="cuda") for b in mgr.batches()]
    mgr.step_sequence_all(DT, meas, use_graph=0, poses=bufs)
    out["pop0"], out["pop1"] = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    mgr.close()
    return out


def _ab_zigzag_child(path):
    np.savez(path, **_ab_zigzag_scenario())
    print("pose scenario ok")


@pytest.mark.parametrize("env", ["TE_PINGPONG_MIN_MB", "TE_ZIGZAG_MIN_MB"])
def test_poses_of_ab_and_zigzag_ticks_equal_in_place_ticks(tmp_path, env):
    """Case 6: a child process with every eager tick an A -> B tick (TE_PINGPONG_MIN_MB=0), one with every tick zig-zagging
    (TE_ZIGZAG_MIN_MB=0): the poses equal those of in-place, forward ticks in this process bit for bit."""
    path = str(tmp_path / "poses.npz")
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    e[env] = "0"
    p = subprocess.run([sys.executable, "-c", "import test_gpu_pose_stream as t; t._ab_zigzag_child(%r)" % path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "pose scenario ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    child = np.load(path)
    here = _ab_zigzag_scenario()
    for k, v in here.items():
        np.testing.assert_array_equal(child[k], v, err_msg=k)
        assert not np.isnan(v).any()


def test_recorded_graphs_keep_their_own_pose_buffers(models):
    """Case 7: two recorded sequences that differ only in their pose buffer are two graphs, each writing into its own buffer."""
    name, dtype, N, ticks = "uniform_velocity", "f64", 130, 4
    p0, meas, soa, mask, has = _inputs(name, dtype, N, ticks, 9, N)
    ids = np.arange(N, dtype=np.uint32)
    soa3 = torch.cat([soa, soa, soa])
    has3 = torch.cat([has, has, has])
    want, _, _ = _twin_poses(model_path(name), dtype, 0, ids, p0, soa3, has3)
    mgr = te.TargetManager(model_path(name), dtype=dtype)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    A = torch.full((ticks, 7, N), float("nan"), dtype=torch.float64, device="cuda")
    B = torch.full((ticks, 7, N), float("nan"), dtype=torch.float64, device="cuda")
    b.step_sequence(DT, soa, has, use_graph=True, poses=A)        # ticks 0-3 -> A
    torch.cuda.synchronize()
    a1 = A.clone()
    b.step_sequence(DT, soa, has, use_graph=True, poses=B)        # ticks 4-7 -> B (a second graph)
    torch.cuda.synchronize()
    assert torch.equal(A, a1), "the second graph wrote into the first one's buffer"
    b1 = B.clone()
    b.step_sequence(DT, soa, has, use_graph=True, poses=A)        # ticks 8-11 -> A (the first graph again)
    torch.cuda.synchronize()
    assert torch.equal(B, b1)
    np.testing.assert_array_equal(_soa_poses(a1, N), want[0:4])
    np.testing.assert_array_equal(_soa_poses(b1, N), want[4:8])
    np.testing.assert_array_equal(_soa_poses(A, N), want[8:12])
    mgr.close()


def test_columns_follow_slot_ids_after_erase(models):
    """Case 8: after a third of the targets is erased, column j is the pose of target_batch_slot_ids()[j]."""
    name, dtype, N, ticks = "angular_velocities", "f64", 300, 3
    p0, meas, soa, mask, has = _inputs(name, dtype, N, ticks, 13, N)
    ids = np.arange(N, dtype=np.uint32) + 1000
    mgr = te.TargetManager(model_path(name), dtype=dtype)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    b.step(DT, soa[0])
    assert mgr.erase_batch(ids[::3]) == len(ids[::3])
    n = b.size
    slot_ids = b.slot_ids()
    assert n == N - len(ids[::3]) and not np.isin(slot_ids, ids[::3]).any()
    buf = torch.full((1, 7, N), float("nan"), dtype=torch.float64, device="cuda")
    b.step_sequence(DT, soa[1:], has[1:], poses=buf)               # tick_stride 0: the last tick's poses
    torch.cuda.synchronize()
    got = _soa_poses(buf, n)[0]
    pose, _, _, found = mgr.get_est_batch(slot_ids)
    assert found.all()
    np.testing.assert_array_equal(got, pose)
    mgr.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["coupled", "classes"])
def test_fallback_layouts(models, kind, dtype):
    """Case 9: a coupled-Q batch (automatic layout: the dense kernel) and a 3-class batch: step + pose writer per tick, bit-equal
    to the twin (eager, recorded and fused) and within the oracle's tolerance."""
    name, N = "angular_rates", 211
    m = models[name]
    p0, meas, soa, mask, has = _inputs(name, dtype, N, TICKS, 21, N + 3)
    ids = np.arange(N, dtype=np.uint32)
    if kind == "coupled":
        c = coupled(m)
        kw = dict(QRP=(c["Q"], c["R"], c["P"], m["model"]))
        want_o = _oracle_poses(m, dtype, p0, meas, mask, Q=c["Q"], R=c["R"], P0=c["P"])
    else:
        scale = np.array([1.0, 2.0, 0.5])
        Q = np.stack([m["Q"] * s for s in scale]); R = np.stack([m["R"] * s for s in scale]); P0 = np.stack([m["P"]] * 3)
        class_of = (np.arange(N) % 3).astype(np.uint32)
        kw = dict(classes=(Q, R, P0, class_of, m["model"]))
        want_o = {s: np.zeros((N, 7)) for s in ORACLE_TICKS}
        for k in range(3):
            sel = class_of == k
            o = _oracle_poses(m, dtype, p0[sel], meas[:, sel], mask[:, sel], Q=Q[k], R=R[k], P0=P0[k])
            for s in ORACLE_TICKS:
                want_o[s][sel] = o[s]
    want, _, _ = _twin_poses(model_path(name), dtype, 0, ids, p0, soa, has, **kw)
    _check_oracle(want, want_o, dtype, "%s %s twin" % (kind, dtype))
    for form in ("eager", "graph", "fused"):
        mgr = _manager(model_path(name), dtype, 0, kw)
        _init(mgr, ids, p0, **kw)
        b = mgr.batches()[0]
        if kind == "coupled":
            assert b.layout in ("full", "symmetric_packed")
        else:
            assert b.num_classes == 3
        buf = torch.full((TICKS, 7, N + 3), float("nan"), dtype=torch.float64, device="cuda")
        if form == "fused":
            b.step_fused(DT, soa, has, poses=buf)
        else:
            b.step_sequence(DT, soa, has, use_graph=form == "graph", poses=buf)
        got = _soa_poses(buf, N)
        np.testing.assert_array_equal(got, want, err_msg="%s %s %s" % (kind, dtype, form))
        _check_oracle(got, want_o, dtype, "%s %s %s" % (kind, dtype, form))
        mgr.close()


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_acceleration", "f64", 3), ("angular_velocities", "f32", 101)])
def test_dense_layouts_with_poses_and_the_fused_query(models, name, dtype, lanes):
    """Case 9b: a batch of the dense kernel in a step_sequence_all with the own-time sphere query and a pose stream -- the QUERY
    step kernel, then the pose writer, per tick.  65 targets (a wavefront and one lane), 3 ticks, target 7 without a measurement
    on tick 2: every tick's poses within the oracle's output tolerance, the state within the parity tolerance, the query results
    the bits of the stand-alone query on the final state."""
    m = models[name]
    N, ticks = 65, 3
    p0, meas = synth_stream(name, N, ticks, seed=41)
    mask = np.ones((ticks, N), np.uint8)
    mask[1, 7] = 0
    tdt = torch.float64 if dtype == "f64" else torch.float32
    soa = torch.zeros((ticks, 7, N + 3), dtype=tdt, device="cuda")
    soa[:, :, :N] = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).to("cuda").to(tdt)
    has = torch.from_numpy(mask).cuda()
    origin, radius = np.array([0.5, -0.25, 0.1]), 6.0
    ids = np.arange(N, dtype=np.uint32)
    mgr = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=lanes)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    assert b.layout in ("full", "symmetric_packed") and not mgr.population_tick()
    buf = torch.full((ticks, 7, N + 3), float("nan"), dtype=torch.float64, device="cuda")
    delta = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    qpose = torch.full((N, 7), float("nan"), dtype=torch.float64, device="cuda")
    mgr.step_sequence_all(DT, [soa], has_meas=[has], query=(origin, radius, [delta], [qpose]), use_graph=0, poses=[buf])
    torch.cuda.synchronize()
    got = _soa_poses(buf, N)
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, DT, dtype=dtype)
    for s in range(ticks):
        orc.step(DT, meas[s], mask[s])
        print("tick %d: worst pose error %.3g (tolerance %.3g)" % (s + 1, np.abs(got[s] - orc.pose()).max(), TOL[dtype]["out_atol"]))
        np.testing.assert_allclose(got[s], orc.pose(), atol=TOL[dtype]["out_atol"], rtol=0, err_msg="tick %d" % (s + 1))
    check_state(mgr, ids, orc, dtype, "%s %s %d" % (name, dtype, lanes))
    d1, p1 = b.intersect_sphere(origin, radius)
    np.testing.assert_array_equal(delta.cpu().numpy(), d1.cpu().numpy())
    np.testing.assert_array_equal(qpose.cpu().numpy(), p1.cpu().numpy())
    mgr.close()


def test_bad_pose_streams_are_refused_and_launch_nothing(models):
    """Case 10: ld < size and 0 < tick_stride < 7 ld return < 0 with an error message; state and buffer are untouched."""
    import ctypes as C
    from target_estimation_amd import capi
    lib = capi.lib()
    name, dtype, N = "uniform_acceleration", "f64", 100
    p0, meas, soa, mask, has = _inputs(name, dtype, N, 2, 4, N)
    ids = np.arange(N, dtype=np.uint32)
    mgr = te.TargetManager(model_path(name), dtype=dtype)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    x0, P0 = mgr.get_state_batch(ids)
    buf = torch.full((2, 7, N), float("nan"), dtype=torch.float64, device="cuda")
    for ld, stride, ring in ((N - 1, 7 * N, 0), (N, 7 * N - 1, 0), (N, 1, 0), (N, -7 * N, 0), (N, 7 * N, -1)):
        ps = capi.PoseStream(buf.data_ptr(), ld, stride, ring)
        rc = lib.target_batch_step_sequence_poses(b._h, 2, DT, soa.data_ptr(), soa.stride(0), soa.stride(1), None, 0, 0, C.byref(ps), 0)
        assert rc < 0 and "pose stream" in capi.last_error()
        rc = lib.target_batch_step_fused_poses(b._h, 2, DT, soa.data_ptr(), soa.stride(0), soa.stride(1), None, 0, C.byref(ps))
        assert rc < 0 and "pose stream" in capi.last_error()
    with pytest.raises(RuntimeError, match="pose stream"):
        b.step_sequence(DT, soa, poses=torch.full((2, 7, N - 1), float("nan"), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    x1, P1 = mgr.get_state_batch(ids)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(P1, P0)
    assert torch.isnan(buf).all()
    mgr.close()
    # the manager-level call checks every batch's stream before it enqueues anything
    mgr, meas, ids2 = _pop_manager(models, [("angular_rates", 300), ("uniform_velocity", 200)], "f64", 2, 3)
    xs = [mgr.get_state_batch(i) for i in ids2]
    # (the second batch's stream: 200 columns per row in the tensor's shape, rows only 150 apart -- ld 150 < 200)
    bad = [torch.full((2, 7, 300), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((2 * 7 * 150 + 50,), float("nan"), dtype=torch.float64, device="cuda").as_strided((2, 7, 200), (7 * 150, 150, 1))]
    with pytest.raises(RuntimeError, match="pose stream"):
        mgr.step_sequence_all(DT, meas, use_graph=0, poses=bad)
    torch.cuda.synchronize()
    for i, (x, P) in zip(ids2, xs):
        x1, P1 = mgr.get_state_batch(i)
        np.testing.assert_array_equal(x1, x)
        np.testing.assert_array_equal(P1, P)
    assert all(torch.isnan(t).all() for t in bad)
    mgr.close()


def test_full_size_cfg4_1gpu_poses(models):
    """Case 11: cfg4_1gpu (500 000 angular-rates + 500 000 angular-velocities targets, fp64), five population ticks with the pose
    stream: every pose bit-equal to step_sequence_all tick by tick followed by get_est_dev per batch."""
    parts, dtype, ticks = [("angular_rates", 500000), ("angular_velocities", 500000)], "f64", 5
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 2024)
    want = [[] for _ in parts]
    for s in range(ticks):
        mgr.step_sequence_all(DT, [m[s:s + 1] for m in meas], use_graph=0)
        for i, b in enumerate(mgr.batches()):
            want[i].append(b.get_est(twist=False, acc=False)[0].cpu().numpy())
    mgr.close()
    mgr, meas, ids = _pop_manager(models, parts, dtype, ticks, 2024)
    assert mgr.population_tick()
    bufs = [torch.full((ticks, 7, b.size), float("nan"), dtype=torch.float64, device="cuda") for b in mgr.batches()]
    mgr.step_sequence_all(DT, meas, use_graph=0, poses=bufs)
    torch.cuda.synchronize()
    for i, b in enumerate(mgr.batches()):
        np.testing.assert_array_equal(_soa_poses(bufs[i], b.size), np.stack(want[i]))
    mgr.close()
