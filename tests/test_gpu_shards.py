"""One TargetManager over several shards (target_manager_set_devices) against a one-shard manager fed the same calls, and
target_manager_get_est_all_by_id (outputs_rows_kernel).  Logical shards on device 0 run the same code as shards on
different devices."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import MODEL_FILES, ROOT, model_path

pytestmark = pytest.mark.gpu

SHARDINGS = [[0, 0, 0], [0, 0]]
DT = 0.004


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _mgr(name, dtype="f64", devices=None):
    import target_estimation_amd as te
    return te.TargetManager(model_path(name), dtype=dtype, devices=devices)


def _poses(rng, n):
    p = np.zeros((n, 7))
    p[:, :3] = rng.normal(size=(n, 3))
    p[:, 6] = 1.0
    return p


def _meas(rng, n, tick):
    m = np.zeros((n, 7))
    m[:, :3] = rng.normal(scale=0.05, size=(n, 3)) + 0.01 * tick
    a = rng.normal(scale=0.02, size=(n, 3))                    # a small rotation as a unit quaternion
    m[:, 3:6] = np.sin(a / 2)
    m[:, 6] = np.sqrt(np.maximum(0.0, 1.0 - (m[:, 3:6] ** 2).sum(1)))
    return m


def _feed(m, seed):
    """ragged creations (batched and one by one through the reference's init), by-id updates in random order with a
    has_meas mask, per-target calls, erase / erase_batch and re-creation; the same calls for every manager"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(1, 400, dtype=np.uint32))[:150]
    m.init_batch(ids[:37], DT, 0.0, _poses(rng, 37))
    m.init_batch(ids[37:100], DT, 0.0, _poses(rng, 63))
    for i in ids[100:113]:
        m.init(int(i), DT, 0.0, _poses(rng, 1)[0])
    live = list(ids[:113])
    for tick in range(12):
        order = rng.permutation(np.array(live, dtype=np.uint32))
        has = (rng.random(len(order)) < 0.8).astype(np.uint8)
        m.update_batch(order, DT, _meas(rng, len(order), tick), has)
        for i in order[:5]:
            m.update(int(i), DT, _meas(rng, 1, tick)[0])
        m.update(int(order[5]), DT)
        if tick == 4:
            m.erase(int(live[3]))
            m.erase_batch(np.array(live[10:30:3], dtype=np.uint32))
            gone = {live[3]} | set(live[10:30:3])
            live = [i for i in live if i not in gone]
        if tick == 7:   # re-creation of erased ids and new ones, across shard borders
            back = np.array(sorted(set(ids[:113]) - set(live))[:5] + list(ids[113:130]), dtype=np.uint32)
            m.init_batch(back, DT, 0.0, _poses(rng, len(back)))
            live += list(back)
    return np.array(sorted(live), dtype=np.uint32)


@pytest.mark.parametrize("devices", SHARDINGS, ids=["3shards", "2shards"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(MODEL_FILES))
def test_sharded_equals_one_shard(name, dtype, devices):
    _torch()
    ref, sh = _mgr(name, dtype), _mgr(name, dtype, devices)
    assert sh.num_shards == len(devices) and ref.num_shards == 1
    live = _feed(ref, 5)
    assert np.array_equal(_feed(sh, 5), live)
    assert np.array_equal(sh.getAvailableTargets(), ref.getAvailableTargets())
    assert np.array_equal(sh.getAvailableTargets(), live) and sh.size() == ref.size() == len(live)
    assert len({sh.shard_of(int(i)) for i in live}) == len(devices)        # every shard holds targets
    assert sh.shard_of(100000) == -1
    x1, P1 = ref.get_state_batch(live)
    x2, P2 = sh.get_state_batch(live)
    assert np.array_equal(x1, x2) and np.array_equal(P1, P2)
    e1, e2 = ref.get_est_batch(live), sh.get_est_batch(live)
    for a, b in zip(e1, e2):
        assert np.array_equal(a, b)
    for i in live[:20]:   # the ten symbols' getters
        (o1, p1), (o2, p2) = ref.getTargetPose(int(i)), sh.getTargetPose(int(i))
        assert o1 and o2 and np.array_equal(p1, p2)
        assert np.array_equal(ref.getTargetTwist(int(i))[1], sh.getTargetTwist(int(i))[1])
        assert ref.getNumberMeasurements(int(i)) == sh.getNumberMeasurements(int(i))
        assert abs(ref.getTime(int(i)) - sh.getTime(int(i))) <= 1e-12
    t1 = 0.3
    a1, a2 = ref.get_est_batch(live, t1=t1), sh.get_est_batch(live, t1=t1)
    tol = 1e-9 if dtype == "f64" else 1e-3
    for a, b in zip(a1[:3], a2[:3]):
        assert np.allclose(a, b, rtol=tol, atol=tol)
    ref.close(); sh.close()


def _matrices(name):
    m = _mgr(name)
    m.init(1, DT, 0.0, [0, 0, 0, 0, 0, 0, 1])
    Q, R, P0 = m.getModelMatrices(1)
    m.close()
    return Q, R, P0


def _mixed(devices, n_uv=300, n_ua=200):
    """uniform_velocity (default model) + uniform_acceleration (typed): two batches per shard"""
    import target_estimation_amd as te
    m = _mgr("uniform_velocity", devices=devices)
    rng = np.random.default_rng(3)
    ids = rng.permutation(np.arange(n_uv + n_ua, dtype=np.uint32) * 3 + 1)
    m.init_batch(ids[:n_uv], DT, 0.0, _poses(rng, n_uv))
    Q, R, P0 = _matrices("uniform_acceleration")
    m.init_batch(ids[n_uv:], DT, 0.0, _poses(rng, n_ua), type=te.UNIFORM_ACCELERATION, Q=Q, R=R, P0=P0)
    return m, np.sort(ids)


def _batch_meas(torch, m, ticks, seed):
    """per-batch measurement tensors [ticks, 7, n] built from per-id measurements, so that every manager sees the same"""
    out = []
    for b in m.batches():
        ids = b.slot_ids()
        t = np.zeros((ticks, 7, len(ids)))
        for j, i in enumerate(ids):
            r = np.random.default_rng(int(i) * 1000 + seed)
            t[:, :3, j] = r.normal(scale=0.05, size=(ticks, 3))
            t[:, 6, j] = 1.0
        out.append(torch.tensor(t, dtype=torch.float64, device="cuda"))
    return out


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("devices", SHARDINGS, ids=["3shards", "2shards"])
def test_step_sequence_all_and_population_tick(devices, use_graph):
    torch = _torch()
    ref, ids = _mixed(None)
    sh, ids2 = _mixed(devices)
    assert np.array_equal(ids, ids2)
    assert sh.population_tick() == ref.population_tick()
    nb = sh._lib.target_manager_num_batches(sh.handle)
    assert nb == 2 * len(devices)
    assert [sh.batch_shard(i) for i in range(nb)] == sorted(sh.batch_shard(i) for i in range(nb))   # shard-major
    assert sh.batch_shard(nb) == -1 and sh.shard_device(0) == 0 and sh.shard_device(len(devices)) == -1
    for m in (ref, sh):
        meas = _batch_meas(torch, m, 16, 9)
        m.step_sequence_all(DT, meas, use_graph=use_graph)
        poses = [torch.zeros((16, 7, b.size), dtype=torch.float64, device="cuda") for b in m.batches()]
        m.step_sequence_all(DT, _batch_meas(torch, m, 16, 10), use_graph=use_graph, poses=poses)
        m.synchronize()
        m._poses = poses
    e1, e2 = ref.get_est_batch(ids), sh.get_est_batch(ids)
    for a, b in zip(e1, e2):
        assert np.array_equal(a, b)
    # every target's last pose in the streams equals the getter's
    for m, e in ((ref, e1), (sh, e2)):
        row = {int(i): k for k, i in enumerate(ids)}
        for b, p in zip(m.batches(), m._poses):
            last = p[15].cpu().numpy()
            for j, i in enumerate(b.slot_ids()):
                assert np.array_equal(last[:, j], e[0][row[int(i)]])
    ref.close(); sh.close()


def _alloc_out(torch, n, where):
    if where == "device":
        return torch.full((n, 7), np.nan, dtype=torch.float64, device="cuda")
    return torch.full((n, 7), np.nan, dtype=torch.float64).pin_memory()


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("devices", [None, [0], [0, 0, 0]], ids=["unsharded", "1shard", "3shards"])
def test_get_est_all_by_id(devices, where):
    torch = _torch()
    m, ids = _mixed(devices)
    for step in range(3):
        if step == 1:   # erase by swap and a batched compaction
            m.erase(int(ids[7]))
            m.erase_batch(ids[100:180:2])
        if step == 2:   # re-created ids go back in at their ranks
            m.init_batch(ids[100:140:2], DT, 0.0, _poses(np.random.default_rng(1), 20))
        m.update_all(DT)
        avail = np.array(m.getAvailableTargets(), dtype=np.uint32)
        want = m.get_est_batch(avail)[0]
        out = _alloc_out(torch, len(avail) + 5, where)
        got = m.get_est_all_by_id(out)
        m.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (len(avail), 7)
        assert np.array_equal(got, want)
        assert np.isnan(out[len(avail):].cpu().numpy()).all()     # nothing beyond size() rows
        assert np.array_equal(m.get_est_all_by_id(), want)
    small = _alloc_out(torch, 3, "device")
    assert m._lib.target_manager_get_est_all_by_id(m.handle, small.data_ptr(), 3) == -1
    assert m._lib.target_manager_get_est_all_by_id(m.handle, None, 0) == m.size()
    m.close()


def test_get_est_all_by_id_at_a_million_targets():
    """the cfg4 population (500 000 angular-rates + 500 000 angular-velocities, fp64) on three shards, ids permuted at random"""
    torch = _torch()
    import target_estimation_amd as te
    m = _mgr("angular_rates", devices=[0, 0, 0])
    rng = np.random.default_rng(4)
    n = 1_000_000
    ids = rng.permutation(np.arange(n, dtype=np.uint32) * 2 + 1)
    m.init_batch(ids[: n // 2], DT, 0.0, _poses(rng, n // 2))
    Q, R, P0 = _matrices("angular_velocities")
    m.init_batch(ids[n // 2:], DT, 0.0, _poses(rng, n - n // 2), type=te.ANGULAR_VELOCITIES, Q=Q, R=R, P0=P0)
    m.update_all(DT)
    avail = np.array(m.getAvailableTargets(), dtype=np.uint32)
    want = m.get_est_batch(avail)[0]
    out = _alloc_out(torch, n, "device")
    assert m.get_est_all_by_id(out).shape[0] == n
    m.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    m.close()


@pytest.mark.parametrize("devices", SHARDINGS, ids=["3shards", "2shards"])
def test_intersections_equal_one_shard(devices):
    _torch()
    from target_estimation_amd import capi
    ref, sh = _mgr("uniform_acceleration"), _mgr("uniform_acceleration", devices=devices)
    live = _feed(ref, 8)
    _feed(sh, 8)
    origin, radius, t1 = [0.5, 0.2, -0.1], 1.5, 0.2
    for a, b in zip(ref.intersect_batch(live, t1, origin, radius), sh.intersect_batch(live, t1, origin, radius)):
        assert np.array_equal(a, b)
    for a, b in zip(ref.intersect_converged_batch(live, t1, 0.1, 0.1, origin, radius, 20),
                    sh.intersect_converged_batch(live, t1, 0.1, 0.1, origin, radius, 20)):
        assert np.array_equal(a, b)
    lib = capi.lib()
    o = np.array(origin)
    op = o.ctypes.data_as(capi.c_double_p)
    sv = [lib.target_intersection_solver_new(m.handle, 30) for m in (ref, sh)]
    try:
        for i in live[:25]:
            d = [lib.target_intersection_solver_get_time_with_sphere(s, int(i), t1, op, radius) for s in sv]
            assert d[0] == d[1]
            p = [np.zeros(7), np.zeros(7)]
            c = [lib.target_intersection_solver_get_pose_with_sphere(s, int(i), t1, 0.1, 0.1, op, radius, q.ctypes.data_as(capi.c_double_p))
                 for s, q in zip(sv, p)]
            assert c[0] == c[1] and np.array_equal(p[0], p[1])
    finally:
        for s in sv:
            lib.target_intersection_solver_delete(s)
    ref.close(); sh.close()


def test_rosbag_replay_through_ingest_on_two_shards():
    _torch()
    import target_estimation_amd as te
    path = os.path.join(ROOT, "tests", "golden", "multiple_targets_tf.npz")
    if not os.path.exists(path):
        pytest.skip("no rosbag fixture")
    a = np.load(path)
    recv, stamp, pose = a["recv_time"], a["stamp"], a["pose"]
    child = [c.decode() for c in a["child_frame_id"]]
    outs = []
    for devices in (None, [0, 0]):
        m = _mgr("uniform_velocity", devices=devices)
        ing = te.MeasurementIngest(m, token="target")
        rows, k, t = [], 0, float(recv[0])
        while k < len(recv):
            t += 0.01
            while k < len(recv) and recv[k] <= t:
                ing.push_named(child[k], float(stamp[k]), pose[k])
                k += 1
            rows.append(ing.tick(0.01, t))
        outs.append(rows)
        ing.close(); m.close()
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_refusals_leave_the_manager_usable():
    torch = _torch()
    from target_estimation_amd import capi
    lib = capi.lib()
    m = _mgr("uniform_velocity")
    devs = (C.c_int * 3)(0, 0, 0)
    assert lib.target_manager_set_devices(m.handle, devs, 0) == -1 and b"at least one" in lib.target_manager_last_error()
    bad = (C.c_int * 2)(0, torch.cuda.device_count())
    assert lib.target_manager_set_devices(m.handle, bad, 2) == -1 and b"out of range" in lib.target_manager_last_error()
    assert m.num_shards == 1
    assert lib.target_manager_set_devices(m.handle, devs, 3) == 0 and m.num_shards == 3
    m.init_batch(np.arange(1, 31, dtype=np.uint32), DT, 0.0, _poses(np.random.default_rng(0), 30))
    assert lib.target_manager_set_devices(m.handle, devs, 2) == -1 and b"already holds targets" in lib.target_manager_last_error()
    assert m.num_shards == 3
    spec = (capi.BatchSequence * 3)()
    assert lib.target_manager_live_start_all(m.handle, DT, C.cast(spec, C.c_void_p), 3, 0, 10, 1.0, 0, None, 0.0) == -1
    assert b"more than one shard" in lib.target_manager_last_error()
    counts = (C.c_long * 1)(30)
    assert lib.target_manager_gather_pose_begin(m.handle, None, 0, counts, None) == -1
    assert b"more than one shard" in lib.target_manager_last_error()
    assert lib.target_manager_set_stream(m.handle, None) == -1 and b"more than one shard" in lib.target_manager_last_error()
    assert lib.target_manager_set_shard_stream(m.handle, 1, None) == 0
    assert lib.target_manager_set_shard_stream(m.handle, 3, None) == -1
    assert lib.target_manager_get_batch_of_type(m.handle, 3) is None and b"more than one shard" in lib.target_manager_last_error()
    with pytest.raises(ValueError):
        m.get_est_all_by_id(torch.zeros((30, 7), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        m.get_est_all_by_id(torch.zeros((7, 30), dtype=torch.float64, device="cuda").t())
    m.update_all(DT)
    assert m.size() == 30 and np.array_equal(m.getAvailableTargets(), np.arange(1, 31))
    assert m.get_est_batch(np.arange(1, 31, dtype=np.uint32))[0].shape == (30, 7)
    m.close()
    # a stream set before set_devices belongs to one device: refused, the manager stays unsharded on that stream
    m = _mgr("uniform_velocity")
    st = torch.cuda.Stream()
    m.set_stream(st.cuda_stream)
    assert lib.target_manager_set_devices(m.handle, devs, 2) == -1 and b"set_stream" in lib.target_manager_last_error()
    assert m.num_shards == 1
    m.set_stream(None)
    assert lib.target_manager_set_devices(m.handle, devs, 2) == 0 and m.num_shards == 2
    assert lib.target_manager_get_batch_of_type(m.handle, 3) is None
    m.close()


def _log_population(m, n, seed):
    """uniform_velocity (default) + uniform_acceleration (typed) targets, interleaved ids, a few by-id ticks, log() after each"""
    import target_estimation_amd as te
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(1, n + 1, dtype=np.uint32) * 3)
    k = n // 2
    m.init_batch(ids[:k], DT, 0.0, _poses(rng, k))
    Q, R, P0 = _matrices("uniform_acceleration")
    m.init_batch(ids[k:], DT, 0.0, _poses(rng, n - k), type=te.UNIFORM_ACCELERATION, Q=Q, R=R, P0=P0)
    for tick in range(3):
        order = rng.permutation(ids)
        m.update_batch(order, DT, _meas(rng, n, tick))
        m.log()
    m.erase(int(ids[0]))
    m.update_all(DT)
    m.log()


@pytest.mark.parametrize("n,select", [(40, False), (64, False), (65, False), (100, False), (150, True)])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]], ids=["2shards", "4shards"])
def test_log_directory_equals_unsharded(tmp_path, devices, n, select):
    """target_manager_log decides per-target files or <channel>_all files from the MANAGER's population (or its explicit
    selection), and a sharded manager writes the same files with the same rows as an unsharded one"""
    _torch()
    dirs = []
    for dv in (None, devices):
        d = tmp_path / ("sharded" if dv else "plain")
        d.mkdir()
        m = _mgr("uniform_velocity", devices=dv)
        m.set_log_directory(str(d))
        if select:
            m.set_log_targets(np.arange(3, 3 * 40, 9, dtype=np.uint32))
        _log_population(m, n, 12)
        m.close()
        dirs.append(d)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert ("est_pose_all" in names) == (n > 64 and not select)
    if select or n <= 64:
        assert len(names) == 7 * (len(np.arange(3, 3 * 40, 9)) if select else n)
    elif n > 65:
        assert len(names) == 7
    for f in names:
        assert (dirs[0] / f).read_text() == (dirs[1] / f).read_text(), f


@pytest.mark.parametrize("name,dtype", [(m, d) for m in ("uniform_velocity", "uniform_acceleration", "angular_rates", "angular_velocities")
                                        for d in ("f64", "f32")])
def test_sharded_300_ticks_against_the_oracle(models, name, dtype):
    """300 by-id ticks on three shards (random order, masked and predict-only ticks): states at every checkpoint, outputs at
    own time and at t1 held to the f80 oracle by tests/test_gpu_precision.py's criterion, and every target's time to
    tests/test_gpu_clock.py's bound"""
    _torch()
    import target_estimation_amd as te
    from test_gpu_clock import Clock, check_clock
    from test_gpu_precision import CHECK, DT as PDT, _outputs, check_outputs, check_states, edge_inputs, run_oracles, tick_mask
    n = 300
    inp = edge_inputs(models, name, dtype, n)
    ref = run_oracles(inp)
    mgr = te.TargetManager(dtype=dtype, devices=[0, 0, 0])
    ids = np.arange(n, dtype=np.uint32) * 5 + 2
    assert mgr.init_batch(ids, PDT, 0.0, inp["p0"], inp["v0"], inp["a0"], type=inp["model"], Q=inp["Q"], R=inp["R"], P0=inp["P0"]) == n
    assert len({mgr.shard_of(int(i)) for i in ids}) == 3
    clk = Clock(0.0)
    perm = np.random.default_rng(n).permutation(n)
    done = 0
    for c in CHECK:
        for s in range(done, c):
            k = tick_mask(inp, s)
            if isinstance(k, str):
                mgr.update_batch(ids[perm], PDT, inp["meas"][s][perm], np.zeros(n, dtype=np.uint8))
            else:
                mgr.update_batch(ids[perm], PDT, inp["meas"][s][perm], None if k is None else k[perm])
            clk.tick(PDT)
        done = c
        check_states("%s sharded by id" % name, inp, ref, c, *mgr.get_state_batch(ids))
        for i in ids[::37]:
            check_clock("sharded by id", "%s %s tick %d" % (name, dtype, c), mgr.getTime(int(i)), clk)
    check_outputs("%s sharded by id" % name, inp, ref, *_outputs(mgr, ids))
    mgr.close()


def test_plain_c_sharded_drop_in(tmp_path):
    _torch()
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "sharded_drop_in_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "sharded_drop_in_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outs = []
    for arg in ("plain", "0,0", "0,0,0"):
        out = subprocess.run([exe, model_path("uniform_velocity"), arg], capture_output=True, text=True, timeout=300)
        print(out.stdout, out.stderr)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "sharded drop-in test ok" in out.stdout and "Target(7) already exists!" in out.stdout
        assert "Target(9) does not exist!" in out.stdout
        outs.append(out.stdout)
    assert outs[0] == outs[1] == outs[2]
