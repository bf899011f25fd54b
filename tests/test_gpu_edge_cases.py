"""Edge cases and full-size properties of the HIP path (MI355X, `pytest -m gpu`)."""
import os

import numpy as np
import pytest

import oracle
from oracle import np_twin as tw
from conftest import HARNESS_ORDER, model_path, synth_stream
from test_gpu_parity import TOL, check_state, to_soa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")


def test_empty_manager_and_empty_calls():
    mgr = te.TargetManager(model_path("uniform_velocity"))
    assert mgr.size() == 0 and len(mgr.getAvailableTargets()) == 0 and len(mgr.batches()) == 0
    mgr.update_all(0.004)                                   # TargetManager::update(dt) on an empty map
    assert mgr.init_batch(np.zeros(0, np.uint32), 0.004, 0.0, np.zeros((0, 7))) == 0
    assert mgr.update_batch(np.zeros(0, np.uint32), 0.004, np.zeros((0, 7))) == 0
    pose, twist, acc, found = mgr.get_est_batch(np.zeros(0, np.uint32))
    assert pose.shape == (0, 7) and found.shape == (0,)
    assert mgr.update_batch(np.array([5], np.uint32), 0.004, np.zeros((1, 7))) == 0   # unknown id: skipped
    mgr.close()


@pytest.mark.parametrize("name", ["angular_rates", "angular_velocities"])
def test_gimbal_branches_of_the_measurement_conversion(models, name):
    """quatToRpy switches to its alternate solution when |sin pitch| > 0.9999 (geometry.hpp:156-169)."""
    m = models[name]
    dt, N = 0.004, 6
    pitches = [np.pi / 2, -np.pi / 2, np.pi / 2 - 0.005, -np.pi / 2 + 0.005, 1.2, -1.2]
    q = np.array([tw.rpy_to_quat(np.array([0.3, p, -0.4])) for p in pitches])
    p0 = np.concatenate([np.zeros((N, 3)), np.tile([0, 0, 0, 1.0], (N, 1))], 1)
    meas = np.concatenate([np.full((N, 3), 0.01), q], 1)
    ids = np.arange(N, dtype=np.uint32)
    mgr = te.TargetManager(model_path(name))
    mgr.init_batch(ids, dt, 0.0, p0)
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, dt)
    for _ in range(3):
        mgr.update_batch(ids, dt, meas)
        orc.step(dt, meas)
    check_state(mgr, ids, orc, "f64", "gimbal")
    x, _ = mgr.get_state_batch(ids)
    assert abs(x[0, 4]) > 0.5 and x[0, 3] != x[4, 3]         # the branch really changed roll
    mgr.close()


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_zero_and_large_dt(models, name):
    m = models[name]
    N = 40
    p0, meas = synth_stream(name, N, 4, seed=2)
    ids = np.arange(N, dtype=np.uint32)
    mgr = te.TargetManager(model_path(name))
    mgr.init_batch(ids, 0.004, 0.0, p0)
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, 0.004)
    for s, dt in enumerate([0.0, 1.0, 0.004, 0.25]):
        mgr.update_batch(ids, dt, meas[s])
        orc.step(dt, meas[s])
        check_state(mgr, ids, orc, "f64", "dt=%g" % dt)
    assert mgr.getTime(3) == pytest.approx(1.254)
    mgr.close()


@pytest.mark.parametrize("name", ["uniform_velocity", "angular_rates"])
def test_growth_mask_and_per_target_P0(models, name):
    """Targets appended after the batch has been stepped (reallocation, later t0), an all-zero
    has_meas mask == predict-only, and per-target P0 through the typed initialiser."""
    m = models[name]
    n = m["Q"].shape[0]
    dt = 0.004
    rng = np.random.default_rng(4)
    p0a, measa = synth_stream(name, 10, 8, seed=5)
    p0b, measb = synth_stream(name, 700, 8, seed=6)
    P0b = np.stack([m["P"] * rng.uniform(0.5, 2.0) for _ in range(700)])
    mgr = te.TargetManager(model_path(name))
    ida, idb = np.arange(10, dtype=np.uint32), np.arange(100, 800, dtype=np.uint32)
    mgr.init_batch(ida, dt, 0.0, p0a)
    oa = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0a, dt, 0.0)
    for s in range(4):
        mgr.update_batch(ida, dt, measa[s])
        oa.step(dt, measa[s])
    mgr.init_batch(idb, dt, 4 * dt, p0b, type=m["model"], Q=m["Q"], R=m["R"], P0=P0b)   # same Q,R -> same batch
    ob = oracle.OracleBatch(m["model"], m["Q"], m["R"], P0b, p0b, dt, 4 * dt)
    assert len(mgr.batches()) == 1 and mgr.batches()[0].size == 710
    b = mgr.batches()[0]
    both = np.concatenate([measa, measb], 1)
    for s in range(4, 8):
        if s == 6:
            b.step(dt, to_soa(both[s], b), torch.zeros(710, dtype=torch.uint8, device="cuda"))
            oa.step(dt, None); ob.step(dt, None)
        else:
            b.step(dt, to_soa(both[s], b))
            oa.step(dt, measa[s]); ob.step(dt, measb[s])
    check_state(mgr, ida, oa, "f64", "old targets")
    check_state(mgr, idb, ob, "f64", "appended targets")
    assert mgr.getNumberMeasurements(3) == 7 and mgr.getNumberMeasurements(100) == 3
    assert mgr.getTime(3) == pytest.approx(8 * dt) and mgr.getTime(500) == pytest.approx(8 * dt)
    _, P = mgr.get_state_batch(idb[:5])
    assert P.shape == (5, n, n)
    mgr.close()


@pytest.mark.parametrize("name,dtype", [("uniform_velocity", "f64"), ("angular_velocities", "f32")])
def test_sequence_and_graph_equal_single_steps(models, name, dtype):
    """target_batch_step_sequence (plain and hipGraph replay) == the same ticks one call at a time."""
    N, ticks, dt = 500, 16, 0.004
    p0, meas = synth_stream(name, N, ticks, seed=8)
    ids = np.arange(N, dtype=np.uint32)
    out = []
    for mode in ("single", "sequence", "graph"):
        mgr = te.TargetManager(model_path(name), dtype=dtype)
        mgr.init_batch(ids, dt, 0.0, p0)
        b = mgr.batches()[0]
        soa = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).cuda().to(b.torch_dtype()).contiguous()
        if mode == "single":
            for s in range(ticks):
                b.step(dt, soa[s])
            for s in range(ticks):
                b.step(dt, soa[s])
        else:
            b.step_sequence(dt, soa, use_graph=(mode == "graph"))
            b.step_sequence(dt, soa, use_graph=(mode == "graph"))      # second call replays the recorded graph
        out.append(mgr.get_state_batch(ids))
        assert mgr.getNumberMeasurements(7) == 2 * ticks
        assert mgr.getTime(7) == pytest.approx(2 * ticks * dt)
        mgr.close()
    for x, P in out[1:]:
        np.testing.assert_array_equal(x, out[0][0])
        np.testing.assert_array_equal(P, out[0][1])


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_velocity", "f64", 0), ("angular_velocities", "f32", 0),
                                              ("angular_rates", "f64", 6), ("uniform_acceleration", "f32", 101),
                                              ("angular_rates", "f32", 301)])
def test_temporally_fused_launch_equals_single_ticks(models, name, dtype, lanes):
    """target_batch_step_fused (n ticks in one launch, state in registers) == n single ticks, bit for
    bit, including a per-tick has_meas mask, the measurement counter and the clock."""
    N, ticks, dt = 700, 12, 0.004
    p0, meas = synth_stream(name, N, ticks, seed=18)
    ids = np.arange(N, dtype=np.uint32)
    mask = (np.random.default_rng(5).random((ticks, N)) < 0.8).astype(np.uint8)
    out = []
    for mode in ("single", "fused"):
        mgr = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=lanes)
        mgr.init_batch(ids, dt, 0.0, p0)
        b = mgr.batches()[0]
        soa = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).cuda().to(b.torch_dtype()).contiguous()
        hm = torch.from_numpy(mask).cuda()
        if mode == "single":
            for s in range(ticks):
                b.step(dt, soa[s], hm[s])
            for s in range(ticks):
                b.step(dt, soa[s])
        else:
            b.step_fused(dt, soa, hm)
            b.step_fused(dt, soa)
        out.append(mgr.get_state_batch(ids))
        assert mgr.getNumberMeasurements(5) == int(mask[:, 5].sum()) + ticks
        assert mgr.getTime(5) == pytest.approx(2 * ticks * dt)
        mgr.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name,dtype,lanes", [("angular_velocities", "f64", 101), ("angular_rates", "f64", 103)])
def test_fused_request_on_a_layout_without_a_fused_kernel(models, name, dtype, lanes):
    """The dense layouts whose temporally fused kernel would spill serve target_batch_step_fused tick by tick, each tick from
    its own measurement block and mask row.  65 targets (a wavefront and one lane), 3 ticks, target 7 without a measurement on
    tick 2: within the parity tolerance of the oracle, the measurement counter and the clock as for single ticks."""
    N, ticks, dt = 65, 3, 0.004
    m = models[name]
    p0, meas = synth_stream(name, N, ticks, seed=37)
    mask = np.ones((ticks, N), np.uint8)
    mask[1, 7] = 0
    ids = np.arange(N, dtype=np.uint32)
    mgr = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=lanes)
    mgr.init_batch(ids, dt, 0.0, p0)
    b = mgr.batches()[0]
    assert b.layout == "symmetric_packed"
    soa = torch.from_numpy(np.ascontiguousarray(meas.transpose(0, 2, 1))).cuda().to(b.torch_dtype()).contiguous()
    b.step_fused(dt, soa, torch.from_numpy(mask).cuda())
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, dt, dtype=dtype)
    for s in range(ticks):
        orc.step(dt, meas[s], mask[s])
    print("worst x / P error", check_state(mgr, ids, orc, dtype, "%s %s %d" % (name, dtype, lanes)))
    assert mgr.getNumberMeasurements(7) == ticks - 1 and mgr.getNumberMeasurements(8) == ticks
    assert mgr.getTime(7) == pytest.approx(ticks * dt)
    mgr.close()


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_reference_harness_in_fp32(models, harness_stream, name):
    """The reference integration test's stream through the fp32 dense path: the reference's own
    assertions still hold and the state tracks the fp32 oracle."""
    k = HARNESS_ORDER.index(name)
    m = models[name]
    dt = 1.0 / m["frequency"]
    meas = harness_stream[k]
    n_points = meas.shape[0]
    mgr = te.TargetManager(model_path(name), dtype="f32")
    mgr.init_batch([0], dt, 0.0, meas[:1])
    b = mgr.batches()[0]
    orc = oracle.OracleTarget(m["model"], m["Q"], m["R"], m["P"], meas[0], dt, dtype="f32")
    soa = torch.from_numpy(np.ascontiguousarray(meas[:, :, None].transpose(0, 1, 2))).cuda().float().contiguous()  # [T,7,1]
    vel_sum = np.zeros(6)
    block = 500
    for s0 in range(0, n_points, block):
        b.step_sequence(dt, soa[s0:s0 + block])
        for i in range(s0, s0 + block):
            orc.add_measurement(dt, meas[i])
        _, twist, _ = b.get_est(pose=False, acc=False)
        vel_sum += twist[0].cpu().numpy() * block   # coarse mean (block-end samples)
    pose, twist, _, _ = mgr.get_est_batch([0])
    goal = np.array([0.2, 0.3, 0.4])
    np.testing.assert_allclose(pose[0, :3], goal, atol=0.01)
    np.testing.assert_allclose((vel_sum / n_points)[:3], goal / (n_points * dt), atol=0.01)
    if name == "angular_velocities":
        np.testing.assert_allclose(twist[0, 3:], [3.0, 0.01, 0.1], atol=0.01)
    x, P = mgr.get_state_batch([0])
    xo, Po = orc.state()
    # angles reach ~120 rad: one fp32 ulp there is 8e-6, and the filters differ by accumulated rounding
    np.testing.assert_allclose(x, xo, atol=5e-3, rtol=1e-4)
    assert np.abs(P - Po).max() <= 5e-2 * np.abs(Po).max()
    mgr.close()


@pytest.mark.parametrize("wl", ["ar1m", "uv1m", "ar1m_full", "av1m_s201", "cfg2", "cfg3", "av1m", "ar1m64", "av1m64", "ua1m64"])
def test_full_size_properties(models, wl):
    """BASELINE-size batches (10^6 targets): properties that do not need the oracle on every target
    (finite, covariance symmetric to rounding with positive diagonal, slot ids in order, predict-only
    leaves the covariance PSD-growing), plus a 2000-target random sample against the oracle."""
    import bench
    from target_estimation_amd.streams import make_stream
    desc, name, dtype, N, seed = bench.WORKLOADS[wl]
    m = models[name]
    dt, ticks = 0.004, 6
    st = make_stream(te.MODEL_TYPES[name], N, ticks, dt, seed, dtype=dtype)
    ids = np.arange(N, dtype=np.uint32)
    mgr = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=bench.TUNED_LANES.get(wl, 0))
    p0 = st["p0"].cpu().numpy()
    assert mgr.init_batch(ids, dt, 0.0, p0) == N
    b = mgr.batches()[0]
    assert b.size == N
    meas = st["meas"]
    assert meas.dtype == b.torch_dtype()
    for s in range(ticks):
        b.step(dt, meas[s])
    sample = np.sort(np.random.default_rng(0).choice(N, 2000, replace=False)).astype(np.uint32)
    sample[0], sample[-1] = 0, N - 1                                   # incl. the last (ragged for 10^4 / 10^5) tile
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0[sample], dt, dtype=dtype)
    ref = oracle.stream_sample(m["model"], seed, sample, ticks, dt, dtype=dtype)   # the CPU regenerates the keyed stream
    np.testing.assert_array_equal(ref["p0"], p0[sample])
    for s in range(ticks):
        orc.step(dt, ref["meas"][s])
    check_state(mgr, sample, orc, dtype, "sample of %s" % wl)
    pose, twist, acc = b.get_est()
    assert torch.isfinite(pose).all() and torch.isfinite(twist).all() and torch.isfinite(acc).all()
    np.testing.assert_array_equal(b.slot_ids()[::9973], ids[::9973])
    tail = np.arange(N - 3000, N, dtype=np.uint32)                    # includes the last (for 10^5: partial) tile
    x, P = mgr.get_state_batch(tail)
    assert np.isfinite(x).all() and np.isfinite(P).all()
    sym = np.abs(P - P.transpose(0, 2, 1)).max(axis=(1, 2)) / np.abs(P).max(axis=(1, 2))
    assert sym.max() < (1e-12 if dtype == "f64" else 1e-4)
    assert (np.diagonal(P, axis1=1, axis2=2) > 0).all()
    b.step(dt, None)                                                   # predict only: P grows (A P A^T + Q)
    _, P2 = mgr.get_state_batch(tail)
    assert (np.diagonal(P2, axis1=1, axis2=2)[:, :3] >= np.diagonal(P, axis1=1, axis2=2)[:, :3]).all()
    assert mgr.getNumberMeasurements(int(tail[-1])) == ticks
    mgr.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_randomised_schedule_against_oracle(models, seed):
    """Seeded fuzz over everything at once: random model / precision / layout, random SPD Q, R, P0
    (decoupled or coupled), random dt per tick, random masks, and a random mix of dense device
    ticks, by-id batches in random order, queued one-target calls (some targets twice) and
    predict-everything ticks; the state is compared with the oracle at the end of every schedule."""
    rng = np.random.default_rng(seed)
    for trial in range(6):
        name = HARNESS_ORDER[int(rng.integers(4))]
        dtype = "f64" if rng.random() < 0.6 else "f32"
        m = models[name]
        n = m["Q"].shape[0]
        if rng.random() < 0.5:                       # coupled matrices -> dense kernel

            def spd(A, s):
                B = rng.normal(size=A.shape) * s
                d = np.sqrt(np.diag(A))
                return A + (B @ B.T) * np.outer(d, d)
            Q, R, P0 = spd(m["Q"], 0.3), spd(m["R"], 0.3), spd(m["P"], 0.3)
            lanes = 0
        else:
            Q, R, P0 = m["Q"], m["R"], m["P"]
            lanes = int(rng.choice([0, 201, 301] + ([3] if n in (6, 9) else [6])))
        N = int(rng.integers(5, 300))
        steps = 14
        p0, meas = synth_stream(name, N, steps, seed=int(rng.integers(1 << 30)))
        ids = (rng.permutation(5000)[:N]).astype(np.uint32)
        mgr = te.TargetManager(dtype=dtype, lanes_per_target=lanes)
        mgr.init_batch(ids, 0.004, 0.0, p0, type=m["model"], Q=Q, R=R, P0=P0)
        orc = oracle.OracleBatch(m["model"], Q, R, P0, p0, 0.004, dtype=dtype)
        b = mgr.batches()[0]
        for s in range(steps):
            dt = float(rng.choice([0.004, 0.001, 0.02, 0.0]))
            mode = int(rng.integers(4))
            if mode == 0:                            # dense device tick with a mask
                mask = (rng.random(N) < 0.8).astype(np.uint8)
                b.step(dt, to_soa(meas[s], b), torch.from_numpy(mask).cuda())
                orc.step(dt, meas[s], mask)
            elif mode == 1:                          # by-id batch in random order, subset
                sub = rng.permutation(N)[: max(1, N * 2 // 3)]
                mask = (rng.random(len(sub)) < 0.7).astype(np.uint8)
                mgr.update_batch(ids[sub], dt, meas[s][sub], mask)
                for j, i in enumerate(sub):
                    _one(orc, int(i), dt, meas[s][i] if mask[j] else None)
            elif mode == 2:                          # queued one-target calls, some targets twice
                calls = [(int(i), bool(rng.random() < 0.8)) for i in rng.choice(N, size=min(N, 9))]
                for i, has in calls:
                    mgr.update(int(ids[i]), dt, meas[s][i] if has else None)
                    _one(orc, i, dt, meas[s][i] if has else None)
            else:                                    # predict everything (TargetManager::update(dt))
                mgr.update_all(dt)
                orc.step(dt, None)
        x, P = mgr.get_state_batch(ids)
        xo, Po = orc.state()
        t = TOL[dtype]
        scale = np.abs(Po).max(axis=(1, 2), keepdims=True)
        assert np.isfinite(x).all()
        assert (np.abs(x - xo) <= 10 * (t["x_atol"] + t["x_rtol"] * np.abs(xo))).all(), (name, dtype, lanes)
        assert (np.abs(P - Po) / scale).max() <= 10 * t["P_rel"], (name, dtype, lanes)
        mgr.close()


def _one(orc, i, dt, meas_row):
    import ctypes as C
    if meas_row is None:
        orc._f("orc_target_update")(orc._at(i), float(dt))
    else:
        row = np.ascontiguousarray(meas_row, dtype=np.float64)
        orc._f("orc_target_add_measurement")(orc._at(i), float(dt), row.ctypes.data_as(C.POINTER(C.c_double)))


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_acceleration", "f64", 0), ("angular_rates", "f32", 0), ("angular_velocities", "f64", 0),
                                              ("uniform_velocity", "f64", 3), ("angular_rates", "f64", 106), ("angular_rates", "f32", 6),
                                              ("angular_velocities", "f32", 101), ("angular_velocities", "f64", 6)])
def test_getter_table_stays_current(models, name, dtype, lanes):
    """The one-target getters are served from a host table that a flush updates only for the stepped slots:
    after any mix of one-target steps, batch steps, erase (slots move) and re-creation every scalar getter
    must equal the batch handle's dense getter, which always runs the outputs kernel on the device (and so must the by-id
    batch getter, served from the same table at this size).
    A flush of up to one wavefront of queued targets writes the table rows from the step kernel itself (one launch, the
    host spins on a completion flag); a longer queue goes through the outputs kernel: the 3-step and the 15-step
    operations below hit both on the lanes-per-target layouts (10 or 21 targets per wavefront) and the first on the
    thread-per-target ones."""
    rng = np.random.default_rng(21)
    N, dt = 37, 0.004
    p0, meas = synth_stream(name, N, 40, seed=23)
    ids = list(range(100, 100 + N))
    mgr = te.TargetManager(model_path(name), dtype=dtype, lanes_per_target=lanes)
    mgr.init_batch(np.array(ids, dtype=np.uint32), dt, 0.0, p0)

    def check():
        arr = np.array(ids, dtype=np.uint32)
        # the reference: the outputs kernel on the device over every slot (the batch handle's dense getter), rows brought into the
        # order of `ids`.  (The by-id batch getter serves calls of this size from the table itself since round 4: it is held to
        # the same rows below, not used as the reference.)
        b = mgr.batches()[0]
        slot_of = {int(v): k for k, v in enumerate(b.slot_ids())}
        rows = [slot_of[int(v)] for v in ids]
        pose, twist, acc = (x.cpu().numpy()[rows] for x in b.get_est())
        pose_b, twist_b, acc_b, found = mgr.get_est_batch(arr)
        assert found.all()
        np.testing.assert_array_equal(pose_b, pose)
        np.testing.assert_array_equal(twist_b, twist)
        np.testing.assert_array_equal(acc_b, acc)
        for j in rng.permutation(len(ids))[:12]:
            for getter, want in ((mgr.getTargetPose, pose), (mgr.getTargetTwist, twist), (mgr.getTargetAcceleration, acc)):
                ok, got = getter(ids[j])
                assert ok
                np.testing.assert_array_equal(got, want[j])

    check()                                               # fills the table
    for s in range(30):
        op = s % 6
        if op in (0, 1, 2):                               # a few one-target steps, read back at once / later
            for j in rng.choice(len(ids), size=15 if op == 2 else 3, replace=False):
                mgr.update(ids[j], dt, meas[s][j % N] if rng.random() < 0.8 else None)
                if op == 0:
                    mgr.getTargetPose(ids[j])             # flush per target (the reference test's loop)
        elif op == 3:                                     # by-id batch step of a subset
            sub = rng.permutation(len(ids))[:10]
            mgr.update_batch(np.array([ids[j] for j in sub], dtype=np.uint32), dt, meas[s][[j % N for j in sub]])
        elif op == 4:                                     # erase: the last slot moves into the hole
            victim = ids.pop(int(rng.integers(len(ids) - 1)))
            assert mgr.erase(victim)
        else:                                             # a new target appears
            new_id = 1000 + s
            mgr.init(new_id, dt, s * dt, p0[s % N])
            ids.append(new_id)
        check()
    mgr.close()


def test_batched_erase_equals_one_by_one(models, capfd):
    """target_manager_erase_batch (one compaction launch per batch) leaves every survivor exactly as erasing the
    same ids one at a time does; unknown / repeated ids are reported and skipped; stepping continues by id."""
    rng = np.random.default_rng(31)
    names = ["uniform_acceleration", "angular_rates"]
    N, dt = 500, 0.004
    mgrs = []
    for _ in range(2):
        mgr = te.TargetManager(dtype="f64")
        for k, name in enumerate(names):
            m = models[name]
            p0, _ = synth_stream(name, N, 2, seed=41 + k)
            mgr.init_batch(np.arange(N, dtype=np.uint32) + 10000 * k, dt, 0.0, p0, type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"])
        mgrs.append(mgr)
    a, b = mgrs
    all_ids = np.concatenate([np.arange(N, dtype=np.uint32), np.arange(N, dtype=np.uint32) + 10000])
    meas = np.tile([0.1, 0.2, 0.3, 0, 0, 0, 1.0], (len(all_ids), 1)) + rng.normal(0, 0.01, (len(all_ids), 7)) * np.array([1, 1, 1, 0, 0, 0, 0])
    for mgr in mgrs:                                   # some history first, including the convergence gates
        mgr.update_batch(all_ids, dt, meas)
        mgr.intersect_converged_batch(all_ids[:50], dt, 1e-3, 1e-3, np.zeros(3), 1.0)
    victims = rng.permutation(all_ids)[:420]
    victims = np.concatenate([victims, victims[:3], [777777]]).astype(np.uint32)      # repeats and an unknown id
    capfd.readouterr()
    assert a.erase_batch(victims) == 420
    out = capfd.readouterr().out
    assert out.count("does not exist!") == 4 and "Target(777777) does not exist!" in out
    for v in victims[:420]:
        assert b.erase(int(v))
    assert a.size() == b.size() == 2 * N - 420
    left = np.array(a.getAvailableTargets(), dtype=np.uint32)
    np.testing.assert_array_equal(left, np.array(b.getAvailableTargets(), dtype=np.uint32))
    np.testing.assert_array_equal(left, np.setdiff1d(all_ids, victims))
    rows = {int(i): j for j, i in enumerate(all_ids)}
    for step in range(3):
        for k in (0, 1):                               # states are per model (one state size per call)
            sub = left[(left >= 10000) == bool(k)]
            xa, Pa = a.get_state_batch(sub)
            xb, Pb = b.get_state_batch(sub)
            np.testing.assert_array_equal(xa, xb)
            np.testing.assert_array_equal(Pa, Pb)
        pa = a.get_est_batch(left)
        pb = b.get_est_batch(left)
        for u, v in zip(pa, pb):
            np.testing.assert_array_equal(u, v)
        sel = rng.permutation(left)[:300]
        mm = meas[[rows[int(i)] for i in sel]]
        assert a.update_batch(sel, dt, mm) == b.update_batch(sel, dt, mm) == 300
    conv_a = a.intersect_converged_batch(left[:40], 3 * dt, 1e-3, 1e-3, np.zeros(3), 1.0)
    conv_b = b.intersect_converged_batch(left[:40], 3 * dt, 1e-3, 1e-3, np.zeros(3), 1.0)
    for u, v in zip(conv_a, conv_b):
        np.testing.assert_array_equal(u, v)
    assert a.erase_batch(left) == len(left) and a.size() == 0 and len(a.getAvailableTargets()) == 0
    a.close(); b.close()


def test_concurrent_callers_of_the_scalar_abi(models):
    """The reference guards its manager with a mutex (target_manager.cpp:192,...); the mirror must serve several
    threads calling the ten-symbol ABI at once (ctypes releases the GIL).  Targets are independent, so each
    thread's targets must end exactly as in a single-threaded run of the same calls."""
    import threading
    name, dt, T, per, steps = "angular_velocities", 0.004, 4, 5, 60
    p0, meas = synth_stream(name, T * per, steps, seed=51)

    def drive(mgr, ids, errors):
        try:
            for s in range(steps):
                for i in ids:
                    mgr.update(i, dt, meas[s][i] if (s + i) % 7 else None)
                    if (s + i) % 3 == 0:
                        ok, _ = mgr.getTargetPose(i)
                        assert ok
        except Exception as exc:      # surfaced by the main thread
            errors.append(exc)

    results = []
    for threaded in (False, True):
        mgr = te.TargetManager(model_path(name))
        for i in range(T * per):
            mgr.init(i, dt, 0.0, p0[i])
        groups = [list(range(k * per, (k + 1) * per)) for k in range(T)]
        errors = []
        if threaded:
            th = [threading.Thread(target=drive, args=(mgr, g, errors)) for g in groups]
            for t in th:
                t.start()
            for t in th:
                t.join()
        else:
            for g in groups:
                drive(mgr, g, errors)
        assert not errors, errors
        ids = np.arange(T * per, dtype=np.uint32)
        results.append((mgr.get_state_batch(ids), [mgr.getNumberMeasurements(int(i)) for i in ids]))
        mgr.close()
    (xa, Pa), na = results[0]
    (xb, Pb), nb = results[1]
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(Pa, Pb)
    assert na == nb


def test_sequence_over_a_measurement_ring(models):
    """target_batch_step_sequence_ring: n ticks over a ring of r < n measurement ticks (tick s reads entry s % r),
    eagerly and from one recorded graph, equal single steps bit for bit."""
    from target_estimation_amd.streams import make_stream
    name, N, dt, ring, total = "angular_rates", 300, 0.004, 5, 17
    st = make_stream(te.MODEL_TYPES[name], N, ring, dt, 61, availability=0.8)
    res = []
    for mode in ("single", "eager", "graph", "all_eager", "all_graph"):
        mgr = te.TargetManager(model_path(name), dtype="f32")
        mgr.init_batch(np.arange(N, dtype=np.uint32), dt, 0.0, st["p0"].cpu().numpy())
        b = mgr.batches()[0]
        meas = st["meas"].to(b.torch_dtype()).contiguous()
        if mode == "single":
            for _ in range(2):                       # every call starts at ring entry 0
                for s in range(total):
                    b.step(dt, meas[s % ring], st["has_meas"][s % ring])
        elif mode.startswith("all"):                 # the manager-level call takes rings too
            for _ in range(2):
                mgr.step_sequence_all(dt, [meas], has_meas=[st["has_meas"]], use_graph=(mode == "all_graph"), n_ticks=total)
        else:
            for _ in range(2):                       # the second call replays the recorded graph
                b.step_sequence(dt, meas, st["has_meas"], use_graph=(mode == "graph"), n_ticks=total)
        res.append(mgr.get_state_batch(np.arange(N, dtype=np.uint32)) + (mgr.getNumberMeasurements(0), mgr.getTime(0)))
        mgr.close()
    for other in res[1:]:
        np.testing.assert_array_equal(other[0], res[0][0])
        np.testing.assert_array_equal(other[1], res[0][1])
        assert other[2] == res[0][2] and other[3] == pytest.approx(res[0][3])


@pytest.mark.parametrize("name,dtype", [("uniform_acceleration", "f32"), ("angular_velocities", "f64")])
def test_host_fed_soa_step_equals_device_step(models, name, dtype):
    """target_batch_step_host (SoA host rows in the batch precision, only the rows the model reads cross PCIe) ==
    target_batch_step on the same values already on the device, with and without a mask, pinned or pageable."""
    from target_estimation_amd.streams import make_stream
    N, dt, ticks = 777, 0.004, 6
    st = make_stream(te.MODEL_TYPES[name], N, ticks, dt, 71, availability=0.7)
    res = []
    for mode in ("device", "host"):
        mgr = te.TargetManager(model_path(name), dtype=dtype)
        mgr.init_batch(np.arange(N, dtype=np.uint32), dt, 0.0, st["p0"].cpu().numpy())
        b = mgr.batches()[0]
        meas = st["meas"].to(b.torch_dtype()).contiguous()
        for s in range(ticks):
            mask = st["has_meas"][s] if s % 2 else None
            if mode == "device":
                b.step(dt, meas[s], mask)
            else:
                rows = meas[s].cpu()
                if s % 3 == 0:
                    rows = rows.pin_memory()
                if name == "uniform_acceleration" and s % 2:
                    rows = rows[:3].contiguous()             # the linear models only need x, y, z
                b.step_host(dt, rows, None if mask is None else mask.cpu())
        res.append(mgr.get_state_batch(np.arange(N, dtype=np.uint32)) + (mgr.getNumberMeasurements(5),))
        mgr.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def _capture_failure_case():
    """Child process of the test below: runs against libtarget_estimation_amd_testhooks.so (TARGET_ESTIMATION_AMD_LIB)."""
    from conftest import MODEL_FILES
    name, dt, N, ticks = "uniform_acceleration", 0.004, 500, 6
    assert te.capi.LIB.endswith("_testhooks.so")
    p0, meas = synth_stream(name, N, ticks, seed=9)
    ids = np.arange(N, dtype=np.uint32)

    def fresh():
        mgr = te.TargetManager(model_path(name), dtype="f64")
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
        mgr.init_batch(ids, dt, 0.0, p0)
        return mgr, mgr.batches()[0]

    ref, rb = fresh()
    for s in range(ticks):
        rb.step(dt, to_soa(meas[s], rb))
    want = ref.get_state_batch(ids)
    mgr, b = fresh()
    seq = torch.stack([to_soa(meas[s], b) for s in range(ticks)])
    os.environ["TE_TEST_FAIL_IN_CAPTURE"] = "1"
    for call in (lambda: b.step_sequence(dt, seq, use_graph=True), lambda: mgr.step_sequence_all(dt, [seq], use_graph=1)):
        try:
            call()
        except RuntimeError as exc:
            assert "injected failure" in str(exc)
        else:
            raise AssertionError("the injected failure did not surface")
    del os.environ["TE_TEST_FAIL_IN_CAPTURE"]
    # nothing was stepped, nothing is stuck: record + replay now works on both paths
    assert abs(mgr.getTime(0)) < 1e-15
    b.step_sequence(dt, seq[:3], use_graph=True)
    mgr.step_sequence_all(dt, [seq[3:]], use_graph=1)
    got = mgr.get_state_batch(ids)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    torch.cuda.synchronize()
    print("capture failure case ok")


def test_a_failure_inside_stream_capture_leaves_no_capture_behind():
    """Round-1 finding: a launch that throws between hipStreamBeginCapture and EndCapture left the capture stream in
    capture mode.  Both recording sites (one batch: target_batch_step_sequence; all batches:
    target_manager_step_sequence_all) now end and destroy the broken capture before reporting.  The failure is injected
    (TE_TEST_FAIL_IN_CAPTURE) -- by a hook that only the test build of the library contains (csrc/Makefile `testhooks`,
    -DTE_TEST_HOOKS; the product library has no such getenv): a child process loads that build through
    TARGET_ESTIMATION_AMD_LIB; afterwards the same call must record, replay and give the bits of plain single steps."""
    import subprocess
    import sys
    from target_estimation_amd import _build
    lib = _build.build_testhooks()
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TARGET_ESTIMATION_AMD_LIB=lib, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_edge_cases as t; t._capture_failure_case()"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "capture failure case ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    # and the product library does not react to the variable at all
    import ctypes
    blob = open(_build.DEFAULT_LIB, "rb").read()
    assert b"TE_TEST_FAIL_IN_CAPTURE" not in blob and b"TE_TEST_FAIL_IN_CAPTURE" in open(lib, "rb").read()
    del ctypes


@pytest.mark.parametrize("name,dtype", [("uniform_acceleration", "f64"), ("angular_velocities", "f32")])
def test_one_by_one_creations_equal_a_batched_creation(models, name, dtype, capfd):
    """TargetManager::init target by target (the reference's only way to create targets; queued here, one init launch per run
    of creations) with everything a caller may put between two creations -- a step of the target just created, a getter, an
    erase, a change of t0, a second model -- against a manager built by init_batch and stepped by update_batch: the same
    bits, the same clocks and counters."""
    m = models[name]
    other = models["uniform_velocity"]
    N, dt = 3000, 0.004
    p0, meas = synth_stream(name, N, 2, seed=5)
    rng = np.random.default_rng(8)
    v0 = rng.uniform(-0.3, 0.3, (N, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    a0 = rng.uniform(-0.1, 0.1, (N, 6)) * 0.1
    ids = (rng.permutation(100000)[:N]).astype(np.uint32)
    t0 = np.where(np.arange(N) < 1000, 0.0, np.where(np.arange(N) < 2200, 1.5, 0.25))     # runs of creations at three clocks
    stepped = np.arange(N) % 37 == 5
    a = te.TargetManager(dtype=dtype)
    for i in range(N):
        a.init(int(ids[i]), dt, float(t0[i]), p0[i], v0[i], a0[i], type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"])
        if stepped[i]:
            a.update(int(ids[i]), dt, meas[0][i])            # a queued step of a queued creation
        if i % 501 == 17:
            assert a.getNumberMeasurements(int(ids[i])) == int(stepped[i])      # a read in the middle of a run
        if i == 1500:                                         # a second model in between (its own batch, its own queue)
            a.init(900001, dt, 0.0, p0[0], np.zeros(6), np.zeros(6), type=other["model"], Q=other["Q"], R=other["R"], P0=other["P"])
        if i == 2000:                                         # an erase in the middle of a run, and the id again
            assert a.erase(int(ids[1990]))
            a.init(int(ids[1990]), dt, float(t0[1990]), p0[1990], v0[1990], a0[1990], type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"])
            if stepped[1990]:
                a.update(int(ids[1990]), dt, meas[0][1990])
    a.init(int(ids[7]), dt, 0.0, p0[8], v0[8], a0[8], type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"])   # an existing id: the reference's message, nothing changes
    assert "already exists" in capfd.readouterr().out
    b = te.TargetManager(dtype=dtype)
    for tt in (0.0, 1.5, 0.25):
        sel = t0 == tt
        assert b.init_batch(ids[sel], dt, tt, p0[sel], v0[sel], a0[sel], type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"]) == sel.sum()
    b.update_batch(ids[stepped], dt, meas[0][stepped])
    assert a.size() == N + 1 and b.size() == N
    for mgr in (a, b):
        mgr.update_batch(ids, dt, meas[1])
    xa, Pa = a.get_state_batch(ids)
    xb, Pb = b.get_state_batch(ids)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(Pa, Pb)
    pa, pb = a.get_est_batch(ids), b.get_est_batch(ids)
    for u, w in zip(pa, pb):
        np.testing.assert_array_equal(u, w)
    for i in list(range(0, N, 211)) + [1990]:
        assert a.getTime(int(ids[i])) == b.getTime(int(ids[i])) == pytest.approx(t0[i] + dt * (1 + stepped[i]), abs=1e-12)
        assert a.getNumberMeasurements(int(ids[i])) == 1 + int(stepped[i])
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, dt, 0.0, v0, a0, dtype=dtype)
    for i in np.nonzero(stepped)[0]:
        _one(orc, int(i), dt, meas[0][i])
    orc.step(dt, meas[1])
    t = TOL[dtype]
    xo, Po = orc.state()
    assert (np.abs(xa - xo) <= t["x_atol"] + t["x_rtol"] * np.abs(xo)).all()
    assert (np.abs(Pa - Po) / np.abs(Po).max(axis=(1, 2), keepdims=True)).max() <= t["P_rel"]
    a.close(); b.close()


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_one_target_call_sequences_against_oracle(models, seed, capfd):
    """Fuzz of the reference's own call pattern -- everything one target at a time, in any order: create (two models, three
    clocks, so that the creation queue breaks into runs), step with and without a measurement, read pose / twist / counter /
    time, erase and re-create.  Each id has its own oracle target; every read is compared when it happens, the state at the
    end.  (Queued creations, queued steps, the getter table, the counter mirror and swap-with-last erase all meet here.)"""
    rng = np.random.default_rng(seed)
    names = ["uniform_velocity", "angular_rates"]
    dtype = "f64"
    t = TOL[dtype]
    mgr = te.TargetManager(dtype=dtype)
    pool = list(range(100, 100 + 260))
    alive = {}            # id -> (oracle target, model name, time, n_meas)
    dt = 0.004
    big = 300 if seed == 13 else 0                       # one run with enough targets for the batch to outgrow a wavefront of queue entries
    for step in range(2600 + big * 4):
        op = rng.random()
        if op < (0.30 if len(alive) < 200 + big else 0.05) or not alive:
            cand = [i for i in pool if i not in alive] or [int(rng.integers(1000, 100000))]
            i = int(rng.choice(cand))
            if i in alive:
                continue
            name = names[int(rng.random() < 0.35)]
            m = models[name]
            t0 = float(rng.choice([0.0, 0.5, 2.0]))
            p0 = np.concatenate([rng.uniform(-5, 5, 3), [0, 0, 0, 1.0]])
            v0 = rng.uniform(-0.5, 0.5, 6) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
            a0 = rng.uniform(-0.1, 0.1, 6) * 0.1
            mgr.init(i, dt, t0, p0, v0, a0, type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"])
            alive[i] = [oracle.OracleTarget(m["model"], m["Q"], m["R"], m["P"], p0, dt, t0, v0, a0, dtype=dtype), name, t0, 0]
            if len(alive) > 200 + big:
                pool.append(i)
        elif op < 0.72:
            i = int(rng.choice(list(alive)))
            o = alive[i]
            d = float(rng.choice([0.004, 0.001, 0.02]))
            if rng.random() < 0.8:
                pose = o[0].pose()[0]
                meas = np.concatenate([pose[:3] + rng.normal(0, 0.01, 3), pose[3:]])
                mgr.update(i, d, meas); o[0].add_measurement(d, meas); o[3] += 1
            else:
                mgr.update(i, d); o[0].update(d)
            o[2] += d
        elif op < 0.92:
            i = int(rng.choice(list(alive)))
            o = alive[i]
            kind = int(rng.integers(4))
            if kind == 0:
                ok, got = mgr.getTargetPose(i)
                assert ok and np.abs(got - o[0].pose()[0]).max() <= t["out_atol"], (step, i)
            elif kind == 1:
                ok, got = mgr.getTargetTwist(i)
                assert ok and np.abs(got - o[0].twist()[0]).max() <= t["out_atol"], (step, i)
            elif kind == 2:
                assert mgr.getNumberMeasurements(i) == o[3], (step, i)
            else:
                assert mgr.getTime(i) == pytest.approx(o[2], abs=1e-9), (step, i)
        elif op < 0.97:
            i = int(rng.choice(list(alive)))
            assert mgr.erase(i)
            del alive[i]
            assert not mgr.getTargetPose(i)[0]
        else:                                            # a sweep of reads over everything alive (the table path for every size)
            for i in list(alive)[:: max(1, len(alive) // 40)]:
                ok, got = mgr.getTargetPose(i)
                assert ok and np.abs(got - alive[i][0].pose()[0]).max() <= t["out_atol"], (step, i)
    assert mgr.size() == len(alive)
    assert sorted(mgr.getAvailableTargets()) == sorted(alive)
    ids = np.array(sorted(alive), dtype=np.uint32)
    for name in names:
        sel = np.array([i for i in ids if alive[int(i)][1] == name], dtype=np.uint32)
        if not len(sel):
            continue
        x, P = mgr.get_state_batch(sel)
        for k, i in enumerate(sel):
            xo, Po = alive[int(i)][0].state()
            assert (np.abs(x[k] - xo[0]) <= t["x_atol"] + t["x_rtol"] * np.abs(xo[0])).all(), (name, int(i))
            assert (np.abs(P[k] - Po[0]) / np.abs(Po[0]).max()).max() <= t["P_rel"], (name, int(i))
    capfd.readouterr()
    mgr.close()
