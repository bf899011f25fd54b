"""The NIS validation gate inside launched ticks (target_batch_step_sequence_gated, target_manager_step_sequence_all_gated;
gate= in manager.py): a measurement whose NIS exceeds nis_max -- or is NaN -- is not folded in, the target is stepped as without
a measurement, and the stream still reports its NIS and innovation.

The defining property, held bit for bit: a gated call leaves every target in the bits the UNGATED call leaves with the mask
has & (0 <= nis <= nis_max), nis read from the gated call's own stream.  Numeric checks are against the gated twin of
tests/gate_ref.py (np_twin.Target per target) with the bounds of tests/innov_stream_ref.py; tests/test_gate_reference.py holds
the conditions these tests rest on (at gamma = 300 every pair is at least 10 bounds from the gate: no pair is excluded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gate_ref
import innov_stream_ref as ref
import oracle
from conftest import HARNESS_ORDER, model_path
from test_gpu_parity import TOL, coupled

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from test_gpu_innov_stream import CASES, POP, _bufs, _init, _manager, _pop_manager, _pop_masks, _read, _soa  # noqa: E402

N, TICKS, DT = gate_ref.N, gate_ref.TICKS, gate_ref.DT
INF = float("inf")


def _counts(mgr, ids):
    return np.array([mgr.getNumberMeasurements(int(i)) for i in ids])


def _run(name, dtype, lanes, p0, soa, has, ids, m, ld, gate=None, use_graph=False, innov=True, kw=None, shared=None):
    """one fresh manager over the stream: (nis, nu) or None, x, P, per-target measurement counters.  shared False / True: a manager
    made with that shared_axes switch, whose batch must then be outside / in the shared-axes form."""
    kw = kw or {}
    mgr = _manager(name, dtype, lanes, **kw, **({} if shared is None else dict(shared_axes=shared)))
    _init(mgr, ids, p0, **kw)
    if shared is not None:
        assert mgr.batches()[0].shared_axes == (1 if shared else 0)
    bufs = _bufs(soa.shape[0], m, ld) if innov else None
    mgr.batches()[0].step_sequence(DT, soa, has, use_graph=use_graph, innov=bufs, gate=gate)
    out = _read(bufs, len(ids)) if innov else None
    torch.cuda.synchronize()
    x, P = mgr.get_state_batch(ids)
    nm = _counts(mgr, ids)
    mgr.close()
    return out, x, P, nm


def _accepted(nis, mask, gamma):
    with np.errstate(invalid="ignore"):
        return mask.astype(bool) & (nis >= 0.0) & (nis <= gamma)


def _gated_equals_masked(name, dtype, lanes, shared=None):
    """the body of test 1: every layout (the gated step kernels for 0 / 201 / 301, the writer's mask row for every other code), eager and
    recorded, at the chi-square 0.99 gate, which rejects a real share of this stream: x and P bit-equal to a fresh manager stepped
    by the plain step_sequence with the mask has & (0 <= nis <= gamma) from the gated call's own stream; the per-target counters
    are the accepted counts; eager and recorded streams bit-equal; padding untouched; NIS -1 exactly where the mask is 0 and
    > gamma on every rejected pair."""
    m, ld = gate_ref.m_of(name), N + 13
    gamma = gate_ref.CHI2_99[m]
    p0, meas, mask, _, _ = gate_ref.stream(name)
    soa, has = _soa(meas, dtype, ld), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32) * 3 + 1
    runs = {g: _run(name, dtype, lanes, p0, soa, has, ids, m, ld, gate=gamma, use_graph=g, shared=shared) for g in (False, True)}
    (nis, nu), x, P, nm = runs[False]
    np.testing.assert_array_equal(runs[True][0][0], nis)
    np.testing.assert_array_equal(runs[True][0][1], nu)
    hasb = mask.astype(bool)
    assert (nis[~hasb] == -1.0).all() and (nu[~hasb] == 0.0).all()
    acc = _accepted(nis, mask, gamma)
    assert (nis[hasb & ~acc] > gamma).all(), "a rejected pair without a NIS above the gate"
    share = (hasb & ~acc).sum() / hasb.sum()
    print("%s %s %d: rejected share of measured pairs %.1f %%" % (name, dtype, lanes, 100 * share))
    assert 0.05 <= share <= 0.60
    _, xm, Pm, nmm = _run(name, dtype, lanes, p0, soa, torch.from_numpy(acc.astype(np.uint8)).cuda(), ids, m, ld, innov=False, shared=shared)
    for g in (False, True):
        np.testing.assert_array_equal(runs[g][1], xm)
        np.testing.assert_array_equal(runs[g][2], Pm)
        np.testing.assert_array_equal(runs[g][3], acc.sum(0))
    np.testing.assert_array_equal(nmm, acc.sum(0))


@pytest.mark.parametrize("name,dtype,lanes", CASES)
def test_gated_equals_masked(name, dtype, lanes):
    """Test 1 on every layout of the innovation tests (in fp64 the codes 0 and 301 are batches in the shared-axes form)."""
    _gated_equals_masked(name, dtype, lanes)


@pytest.mark.parametrize("lanes", [0, 301])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_gated_equals_masked_outside_the_shared_form(name, lanes):
    """Test 1 for fp64 batches kept out of the shared-axes form (shared_axes=False): the gated kernels of the plain layout with
    packed groups, which hold the columns P^-[1:,0] across the decision."""
    _gated_equals_masked(name, "f64", lanes, shared=False)


def _writer_layout(name, dtype):
    """one layout code per (model, precision) whose gate is the writer's mask row"""
    return {"uniform_velocity": 103, "uniform_acceleration": 1, "angular_rates": 106, "angular_velocities": 3}[name]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_against_the_gated_twin(name, dtype):
    """Test 2: gamma = 300 on lanes 0 (fp64: the shared-axes form), 301 and one writer layout: the decisions are the twin's on every
    measured pair, none excluded; nu and NIS within the innovation stream's bound against the gated twin on every tick -- the yaw
    spikes' ticks and the clean ticks behind them included -- and the final x, P within TOL[dtype] as test_gpu_parity compares."""
    m, ld, gamma = gate_ref.m_of(name), N + 13, gate_ref.GAMMA_FAR
    p0, meas, mask, outlier, spikes = gate_ref.stream(name)
    want = gate_ref.reference(name, gamma)
    soa, has = _soa(meas, dtype, ld), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    t = TOL[dtype]
    for lanes in ([0] if dtype == "f64" else []) + [301, _writer_layout(name, dtype)]:
        (nis, nu), x, P, nm = _run(name, dtype, lanes, p0, soa, has, ids, m, ld, gate=gamma)
        what = "%s %s %d gated" % (name, dtype, lanes)
        acc = _accepted(nis, mask, gamma)
        np.testing.assert_array_equal(acc, want["acc"], err_msg=what + ": a decision differs from the twin's")
        ref.check(nu, nis, want, mask, dtype, what)
        np.testing.assert_array_equal(nm, want["acc"].sum(0))
        ex = np.abs(x - want["x"]).max()
        ep = max(np.abs(P[j] - want["P"][j]).max() / np.abs(want["P"][j]).max() for j in range(N))
        print("%s: worst |dx| %.3g, worst |dP| / max|P| %.3g" % (what, ex, ep))
        np.testing.assert_allclose(x, want["x"], atol=t["x_atol"], rtol=t["x_rtol"])
        for j in range(N):
            assert np.abs(P[j] - want["P"][j]).max() <= t["P_rel"] * np.abs(want["P"][j]).max()


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_velocity", "f64", 0), ("uniform_acceleration", "f32", 301), ("angular_rates", "f64", 301),
                                              ("angular_rates", "f32", 201), ("angular_velocities", "f64", 0), ("angular_velocities", "f32", 301),
                                              ("angular_rates", "f64", 6), ("angular_velocities", "f32", 101)])
def test_nan_measurements_are_rejected(name, dtype, lanes):
    """Test 3: x = NaN for one target on tick 5 (angular models: a NaN quaternion for another): that pair is rejected, the stream
    holds NaN there, the final state is finite and bit-equal to the plain run with the pair masked off."""
    m, ld, gamma = gate_ref.m_of(name), N, gate_ref.GAMMA_FAR
    p0, meas, mask, _, _ = gate_ref.stream(name)
    meas, mask = meas.copy(), mask.copy()
    pairs = [(5, 70)] + ([(5, 133)] if m == 6 else [])
    for s, j in pairs:
        mask[s, j] = 1
    meas[5, 70, 0] = np.nan
    if m == 6:
        meas[5, 133, 3:7] = np.nan
    soa, has = _soa(meas, dtype, ld), torch.from_numpy(mask.copy()).cuda()
    ids = np.arange(N, dtype=np.uint32)
    (nis, nu), x, P, nm = _run(name, dtype, lanes, p0, soa, has, ids, m, ld, gate=gamma)
    acc = _accepted(nis, mask, gamma)
    for s, j in pairs:
        assert np.isnan(nis[s, j]) and np.isnan(nu[s, j]).any() and not acc[s, j]
    assert np.isnan(nis).sum() == len(pairs)
    assert np.isfinite(x).all() and np.isfinite(P).all()
    _, xm, Pm, nmm = _run(name, dtype, lanes, p0, soa, torch.from_numpy(acc.astype(np.uint8)).cuda(), ids, m, ld, innov=False)
    np.testing.assert_array_equal(x, xm)
    np.testing.assert_array_equal(P, Pm)
    np.testing.assert_array_equal(nm, nmm)


def _pop_outliers(meas, has, seed):
    """+0.5 m on a Bernoulli(1/12) subset of every batch's measured pairs (CUDA tensors [ticks, 7, ld] / [ticks, n]), in place"""
    rng = np.random.default_rng(seed)
    for t, h in zip(meas, has):
        hit = (rng.random(tuple(h.shape)) < 1.0 / 12.0) & (h.cpu().numpy() != 0)
        axis = rng.integers(0, 3, hit.shape)
        for s, j in zip(*np.nonzero(hit)):
            t[s, axis[s, j], j] += 0.5


def _pop_manager_plain(models, parts, dtype, ticks, seed):
    """test_gpu_innov_stream._pop_manager for a manager kept out of the shared-axes form"""
    from target_estimation_amd.streams import make_stream
    mgr = te.TargetManager(dtype=dtype, shared_axes=False)
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


# (the last case: the fp64 population kept out of the shared-axes form -- the plain fp64 population kernel)
GATE_POP = [(p, d, s, False) for p, d, s in POP] + [(POP[0][0], "f64", False, True)]


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("parts,dtype,shared,plain", GATE_POP)
def test_population_tick(models, parts, dtype, shared, plain, use_graph):
    """Test 4: the one-launch population tick with a gate on every batch, eager and recorded: streams and states bit-equal to
    per-batch gated calls, population_tick() stays true; with a gate on batch 0 only, batch 1 equals its _innov run."""
    ticks, gamma = 6, gate_ref.GAMMA_FAR
    has = _pop_masks(parts, ticks, 5)

    def fresh():
        mgr, meas, ids = (_pop_manager_plain if plain else _pop_manager)(models, parts, dtype, ticks, 77)
        _pop_outliers(meas, has, 6)
        return mgr, meas, ids

    want = {}
    for gates in ((gamma, gamma), (gamma, 0.0)):
        mgr, meas, ids = fresh()
        res = []
        for i, b in enumerate(mgr.batches()):
            bufs = _bufs(ticks, b.meas_dim, b.size + 5)
            b.step_sequence(DT, meas[i], has[i], innov=bufs, gate=gates[i] if gates[i] else None)
            out = _read(bufs, b.size)
            torch.cuda.synchronize()
            res.append((out, mgr.get_state_batch(ids[i]), _counts(mgr, ids[i])))
        want[gates] = res
        mgr.close()
    rejected = sum(((w[0][0] > gamma).sum() for w in want[gamma, gamma]))
    assert rejected > 0, "no pair is rejected: the test does not reach the gate"
    for gates in ((gamma, gamma), (gamma, 0.0)):
        mgr, meas, ids = fresh()
        assert mgr.population_tick()
        bs = mgr.batches()
        bufs = [_bufs(ticks, b.meas_dim, b.size + 5) for b in bs]
        mgr.step_sequence_all(DT, meas, has_meas=has, use_graph=use_graph, innov=bufs, gate=list(gates))
        assert mgr.population_tick()
        if shared is not None:
            assert [b.shared_axes for b in bs] == [1 if shared else 0] * len(bs)
        for i, b in enumerate(bs):
            (wn, wu), (wx, wP), wc = want[gates][i]
            nis, nu = _read(bufs[i], b.size)
            np.testing.assert_array_equal(nis, wn)
            np.testing.assert_array_equal(nu, wu)
            x, P = mgr.get_state_batch(ids[i])
            np.testing.assert_array_equal(x, wx)
            np.testing.assert_array_equal(P, wP)
            np.testing.assert_array_equal(_counts(mgr, ids[i]), wc)
        mgr.close()


@pytest.mark.parametrize("name", ["uniform_velocity", "angular_rates", "angular_velocities"])
def test_shared_form_and_uniform_tiles(models, name):
    """Test 5: 130 fp64 targets with one p0 in the shared-axes form: four clean ticks, one tick with the +0.5 m outlier on targets
    5..39 (the gate splits tile 0 where a mask would), two clean ticks; a twin manager takes the plain call with the mask acc.
    After every phase both are still in the form with the same uniform tiles -- some after phase 1 where the model has them,
    fewer after the split -- and the states are the same bits."""
    dtype, n, m, ticks, gamma = "f64", 130, gate_ref.m_of(name), 7, gate_ref.GAMMA_FAR
    p0, meas, _, _ = ref.stream_and_reference(name, n, ticks, 9)
    p0 = np.tile(p0[:1], (n, 1))
    meas = np.tile(meas[:, :1], (1, n, 1))        # (one trajectory: the innovations of a tick are the same for every target)
    meas[4, 5:40, 1] += 0.5
    soa = _soa(meas, dtype, n)
    ids = np.arange(n, dtype=np.uint32)
    a, t = _manager(name, dtype), _manager(name, dtype)
    _init(a, ids, p0)
    _init(t, ids, p0)
    ab, tb = a.batches()[0], t.batches()[0]
    bufs = _bufs(ticks, m, n)
    seen = []
    for lo, hi in ((0, 4), (4, 5), (5, 7)):
        ab.step_sequence(DT, soa[lo:hi], None, innov=(bufs[0][lo:hi], bufs[1][lo:hi]), gate=gamma)
        torch.cuda.synchronize()
        nis = bufs[0][lo:hi].cpu().numpy()
        acc = (nis >= 0.0) & (nis <= gamma)
        tb.step_sequence(DT, soa[lo:hi], torch.from_numpy(acc.astype(np.uint8)).cuda())
        torch.cuda.synchronize()
        if lo == 4:
            assert not acc[0, 5:40].any() and acc[0, :5].all() and acc[0, 40:].all(), "the outlier tick is not split as intended"
        else:
            assert acc.all(), "a clean pair is rejected"
        assert ab.shared_axes == 1 and tb.shared_axes == 1
        assert ab.uniform_tiles == tb.uniform_tiles
        seen.append(ab.uniform_tiles)
    if name != "angular_velocities":
        assert seen[0] > 0, "no tile became uniform: the test does not reach the uniform-tile path"
        assert seen[1] < seen[0], "the rejected measurements did not split their tile"
    xa, Pa = a.get_state_batch(ids)
    xt, Pt = t.get_state_batch(ids)
    np.testing.assert_array_equal(xa, xt)
    np.testing.assert_array_equal(Pa, Pt)
    np.testing.assert_array_equal(_counts(a, ids), _counts(t, ids))
    a.close()
    t.close()


@pytest.mark.parametrize("name,dtype,lanes", [("uniform_acceleration", "f64", 0), ("angular_rates", "f32", 301), ("angular_velocities", "f64", 201),
                                              ("uniform_velocity", "f32", 3)])
def test_without_a_mask_the_counters_are_the_accepted_counts(name, dtype, lanes):
    """Test 6: has_meas NULL at gamma = 300: n_measurements of every target is its accepted count, the state that of the plain call
    with the mask acc."""
    m, gamma = gate_ref.m_of(name), gate_ref.GAMMA_FAR
    p0, meas, mask, _, _ = gate_ref.stream(name)
    soa = _soa(meas, dtype, N)
    ids = np.arange(N, dtype=np.uint32)
    (nis, nu), x, P, nm = _run(name, dtype, lanes, p0, soa, None, ids, m, N, gate=gamma)
    acc = _accepted(nis, np.ones_like(mask), gamma)
    assert (~acc).sum() > 100 and (nis >= 0).all()
    np.testing.assert_array_equal(nm, acc.sum(0))
    _, xm, Pm, nmm = _run(name, dtype, lanes, p0, soa, torch.from_numpy(acc.astype(np.uint8)).cuda(), ids, m, N, innov=False)
    np.testing.assert_array_equal(x, xm)
    np.testing.assert_array_equal(P, Pm)
    np.testing.assert_array_equal(nm, nmm)


@pytest.mark.parametrize("has_mask", [True, False])
@pytest.mark.parametrize("name,dtype,lanes", [("uniform_velocity", "f64", 0), ("uniform_acceleration", "f32", 201), ("angular_rates", "f64", 0),
                                              ("angular_rates", "f32", 301), ("angular_velocities", "f64", 301), ("angular_velocities", "f32", 201),
                                              ("angular_velocities", "f64", 103)])
def test_an_infinite_gate_is_the_innovation_call(name, dtype, lanes, has_mask):
    """Test 7: nis_max = +inf: streams, state and counters bit-equal to the _innov call -- the two-phase kernels form the bits of
    the one-phase ones."""
    m = gate_ref.m_of(name)
    p0, meas, mask, _, _ = gate_ref.stream(name)
    soa, has = _soa(meas, dtype, N), (torch.from_numpy(mask.copy()).cuda() if has_mask else None)
    ids = np.arange(N, dtype=np.uint32)
    (gn, gu), gx, gP, gc = _run(name, dtype, lanes, p0, soa, has, ids, m, N, gate=INF)
    (wn, wu), wx, wP, wc = _run(name, dtype, lanes, p0, soa, has, ids, m, N)
    for got, want in ((gn, wn), (gu, wu), (gx, wx), (gP, wP), (gc, wc)):
        np.testing.assert_array_equal(got, want)


def test_kept_measured_poses_are_the_accepted_ones():
    """With target_manager_set_keep_measurement the measured pose of a target is its last ACCEPTED measurement: after one tick with
    an outlier on targets 3 and 77 their rows are those of the tick before, every other row is this tick's, and the state is the
    plain call's with the mask acc (a batch that keeps the rows takes the writer's mask row whatever its layout)."""
    name, dtype, n, m, gamma = "angular_rates", "f64", 130, 6, gate_ref.GAMMA_FAR
    p0, meas, _, _ = ref.stream_and_reference(name, n, 4, 9)
    meas = meas.copy()
    meas[3, [3, 77], 2] += 0.5
    soa = _soa(meas, dtype, n)
    ids = np.arange(n, dtype=np.uint32)
    res = []
    for gated in (True, False):
        mgr = _manager(name, dtype)
        mgr.set_keep_measurement(True)
        _init(mgr, ids, p0)
        b = mgr.batches()[0]
        mask = np.ones((4, n), np.uint8)
        if gated:
            bufs = _bufs(4, m, n)
            b.step_sequence(DT, soa, None, innov=bufs, gate=gamma)
            nis, _ = _read(bufs, n)
            acc = _accepted(nis, mask, gamma)
            assert (~acc).sum() == 2 and not acc[3, 3] and not acc[3, 77]
        else:
            mask[3, [3, 77]] = 0
            b.step_sequence(DT, soa, torch.from_numpy(mask).cuda())
        torch.cuda.synchronize()
        res.append((mgr.get_state_batch(ids), np.array([mgr.getMeasuredPose(int(i))[1] for i in (3, 77, 4)]), _counts(mgr, ids)))
        mgr.close()
    for k in (0, 1):
        np.testing.assert_array_equal(res[0][0][k], res[1][0][k])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][2], res[1][2])
    np.testing.assert_allclose(res[0][1][:2, :3], meas[2, [3, 77], :3], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res[0][1][2, :3], meas[3, 4, :3], rtol=0, atol=1e-12)


def test_bad_gates_are_refused_and_launch_nothing(models):
    """Test 8: a negative or NaN nis_max and a gate without a stream, at the batch and at the manager, use_graph 0 / 1: a negative
    return code and a message that names the gate; state and buffers untouched."""
    import ctypes as C
    from target_estimation_amd import capi
    lib = capi.lib()
    name, dtype, n, m = "angular_rates", "f64", 100, 6
    p0, meas, mask, _ = ref.stream_and_reference(name, n, 2, 4)
    soa = _soa(meas, dtype, n)
    ids = np.arange(n, dtype=np.uint32)
    mgr = _manager(name, dtype)
    _init(mgr, ids, p0)
    b = mgr.batches()[0]
    x0, P0 = mgr.get_state_batch(ids)
    nis, nu = _bufs(2, m, n)
    good = capi.InnovStream(nis.data_ptr(), nu.data_ptr(), n, n, m * n, 0)
    no_row = capi.InnovStream(None, nu.data_ptr(), n, n, m * n, 0)
    for use_graph in (0, 1):
        for stream, gate in ((good, -1.0), (good, float("nan")), (None, 11.0), (no_row, 11.0), (None, INF)):
            rc = lib.target_batch_step_sequence_gated(b._h, 2, DT, soa.data_ptr(), soa.stride(0), soa.stride(1), None, 0, 0, None,
                                                      None if stream is None else C.byref(stream), gate, use_graph)
            assert rc < 0 and "gate" in capi.last_error(), (gate, capi.last_error())
    with pytest.raises(RuntimeError, match="gate"):
        b.step_sequence(DT, soa, innov=(nis, nu), gate=-2.0)
    with pytest.raises(RuntimeError, match="gate"):
        b.step_sequence(DT, soa, gate=11.0)
    torch.cuda.synchronize()
    x1, P1 = mgr.get_state_batch(ids)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(P1, P0)
    assert torch.isnan(nis).all() and torch.isnan(nu).all()
    assert (_counts(mgr, ids) == 0).all()
    mgr.close()
    mgr, meas2, ids2 = _pop_manager(models, [("angular_rates", 300), ("uniform_velocity", 200)], "f64", 2, 3)
    xs = [mgr.get_state_batch(i) for i in ids2]
    b0, b1 = _bufs(2, 6, 300), _bufs(2, 3, 200)
    for use_graph in (0, 1):
        for gates, innov in (([11.0, -1.0], [b0, b1]), ([float("nan"), 0.0], [b0, b1]), ([0.0, 11.0], [b0, None]), (11.0, None)):
            with pytest.raises(RuntimeError, match="gate"):
                mgr.step_sequence_all(DT, meas2, use_graph=use_graph, innov=innov, gate=gates)
    torch.cuda.synchronize()
    for i, (x, P) in zip(ids2, xs):
        x1, P1 = mgr.get_state_batch(i)
        np.testing.assert_array_equal(x1, x)
        np.testing.assert_array_equal(P1, P)
    assert all(torch.isnan(t).all() for t in (*b0, *b1))
    mgr.close()


def _ab_zigzag_scenario():
    """gated streams, final states and counters of an eager sequence on a separable fp64 batch and a separable fp32 batch (the
    gated kernels), a coupled-matrix batch (the writer's mask row) and a two-model population tick, at the chi-square gate"""
    from conftest import MODEL_FILES
    models = {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}
    out = {}
    for key, (name, dtype, QRP) in {"sep_f64": ("angular_rates", "f64", False), "sep_f32": ("uniform_acceleration", "f32", False),
                                    "dense": ("angular_velocities", "f64", True)}.items():
        m = gate_ref.m_of(name)
        p0, meas, mask, _, _ = gate_ref.stream(name)
        soa, has = _soa(meas[:7], dtype, N), torch.from_numpy(mask[:7].copy()).cuda()
        ids = np.arange(N, dtype=np.uint32)
        kw = {}
        if QRP:
            c = coupled(models[name])
            kw = dict(QRP=(c["Q"], c["R"], c["P"], models[name]["model"]))
        (nis, nu), x, P, nm = _run(name, dtype, 0, p0, soa, has, ids, m, N, gate=gate_ref.CHI2_99[m], kw=kw)
        assert (nis > gate_ref.CHI2_99[m]).any()
        out[key + "_nis"], out[key + "_nu"], out[key + "_x"], out[key + "_P"], out[key + "_nm"] = nis, nu, x, P, nm
    parts = [("angular_rates", 900), ("uniform_velocity", 800)]
    mgr, meas, ids = _pop_manager(models, parts, "f64", 7, 11)
    bufs = [_bufs(7, b.meas_dim, b.size) for b in mgr.batches()]
    mgr.step_sequence_all(DT, meas, use_graph=0, innov=bufs, gate=[16.812, 11.345])
    torch.cuda.synchronize()
    for i in range(2):
        out["pop%d_x" % i], out["pop%d_P" % i] = mgr.get_state_batch(ids[i])
        out["pop%d_nis" % i], out["pop%d_nu" % i] = bufs[i][0].cpu().numpy(), bufs[i][1].cpu().numpy()
    mgr.close()
    return out


def _ab_zigzag_child(path):
    np.savez(path, **_ab_zigzag_scenario())
    print("gate scenario ok")


@pytest.mark.parametrize("env", ["TE_PINGPONG_MIN_MB", "TE_ZIGZAG_MIN_MB"])
def test_forced_ab_and_zigzag_children(tmp_path, env):
    """Test 9: a fresh child process in which every eager tick that may be is an A -> B tick (TE_PINGPONG_MIN_MB=0), one in which
    every tick zig-zags (TE_ZIGZAG_MIN_MB=0): the gated streams, states and counters equal this process's bit for bit (a gated tick
    runs in place; the zig-zag only reorders the workgroups)."""
    path = str(tmp_path / "gate.npz")
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    e[env] = "0"
    p = subprocess.run([sys.executable, "-c", "import test_gpu_gate as t; t._ab_zigzag_child(%r)" % path], env=e,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "gate scenario ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    child = np.load(path)
    here = _ab_zigzag_scenario()
    for k, v in here.items():
        np.testing.assert_array_equal(child[k], v, err_msg=k)
