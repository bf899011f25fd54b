"""The device build of te_quartic.hpp (v_rcp_f64 + two Newton steps for 1 / d, the device cbrtf, contraction off inside kernels
compiled with contraction on) on the hard sphere scenes of tests/golden/quartic_cases.npz, through every kernel that inlines it,
held to the acceptance rule of tests/test_quartic_cases.py (stated there, with K = 8 and the measured ratios: the kernels' worst
error is 0.122 of 8 eps |want| / min(1, m), one ulp of the crossing time, the oracle's 0.019 -- profiles/quartic_cases_ratios.txt).

Every case is a uniform-acceleration target created with (p, v, a): its state is [p v a] to the bit (asserted), and a query at its
own time solves exactly the fixture's quartic.  A launch takes one sphere, so every path runs once per scene of the fixture and a
case takes its answer from the launch of its own scene.  The standalone kernel is held to the rule; every other path (the indexed
launch, the scalar entries, the other model, the fused queries of the step kernels, the population kernel, recorded launches, the
resident kernels) must give the standalone kernel's bits.  The cases run in the pytest process with the default policies and in
a child process with TE_PINGPONG_MIN_MB=0 TE_ZIGZAG_MIN_MB=0 (A -> B ticks, reversed tile walks), as tests/test_gpu_shared_axes.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MODEL_FILES, model_path
from test_quartic_cases import accept, cases, pose6

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

DT = 0.004
IDENT = [0, 0, 0, 1.0]


def _models():
    import oracle
    return {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}


def _interleaved(cs):
    """an order that deals the families round robin: long-road lanes and lanes Sturm's chain settles share every wavefront"""
    rank = np.zeros(cs.n, dtype=np.int64)
    for f in range(len(cs.family_names)):
        s = np.nonzero(cs.family == f)[0]
        rank[s] = np.arange(len(s)) * 64 // max(1, len(s) // 47 + 1)
    return np.lexsort((cs.family, np.random.default_rng(3).permutation(cs.n), rank))


def _create(models, cs, name="uniform_acceleration", order=None, mats=None, mgr=None, first_id=100, **kw):
    """The cases as targets of model `name`, created in `order` (slot = position in it); returns (manager, ids by case)."""
    m = models[name]
    mats = mats or dict(Q=m["Q"], R=m["R"], P=m["P"])
    if mgr is None:
        mgr = te.TargetManager(dtype=cs.dtype, **kw)
        mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    order = np.arange(cs.n) if order is None else order
    ids = np.arange(cs.n, dtype=np.uint32) + first_id
    p0, _ = pose6(cs.p)
    v0, a0 = pose6(cs.v)[1], pose6(cs.a)[1]
    assert mgr.init_batch(ids[order], DT, 0.0, p0[order], v0[order], a0[order], type=te.MODEL_TYPES[name], Q=mats["Q"], R=mats["R"], P0=mats["P"]) == cs.n
    _assert_state(mgr, cs, ids, name)
    return mgr, ids


def _assert_state(mgr, cs, ids, name="uniform_acceleration"):
    """the state holds p, v, a to the bit (and nothing else that moves the position)"""
    x, _ = mgr.get_state_batch(ids)
    if name == "uniform_acceleration":
        assert np.array_equal(x, np.concatenate([cs.p, cs.v, cs.a], 1))
    else:                                   # angular_rates: [p rpy v rates a alpha]
        want = np.zeros((cs.n, 18))
        want[:, 0:3], want[:, 6:9], want[:, 12:15] = cs.p, cs.v, cs.a
        assert np.array_equal(x, want)


def _slots(b, ids):
    """row of every case in the batch's slot order"""
    slot_of = {int(i): k for k, i in enumerate(b.slot_ids())}
    return np.array([slot_of[int(i)] for i in ids])


def _per_scene(cs, query):
    """query(origin, radius) -> (delta [n], pose [n, 7]) by case; every case from the launch of its own scene"""
    delta, pose = np.full(cs.n, np.nan), np.full((cs.n, 7), np.nan)
    for k, (origin, radius) in enumerate(cs.scenes):
        d, p = query(origin, radius)
        sel = cs.scene == k
        delta[sel], pose[sel] = d[sel], p[sel]
    return delta, pose


def _same(what, got, want):
    for u, v, part in zip(got, want, ("delta", "pose")):
        assert np.array_equal(u, v), "%s: %s differs from the standalone kernel in %d cases, first %s" % (
            what, part, (u != v).reshape(len(u), -1).any(1).sum(), np.nonzero((u != v).reshape(len(u), -1).any(1))[0][:5])


def _standalone(mgr, cs, ids, k=0):
    b = mgr.batches()[k]
    rows = _slots(b, ids)

    def dense(t1):
        def q(origin, radius):
            d, p = b.intersect_sphere(origin, radius, t1=t1)
            return d.cpu().numpy()[rows], p.cpu().numpy()[rows]
        return q
    return _per_scene(cs, dense(None))


def _fused(mgr, cs, idss, use_graph):
    """One predict-only tick with dt = 0 per scene through step_sequence_all with the query: the state keeps its bits, so the
    fused query meets the fixture's quartics.  Returns every batch's answers by case."""
    bs = mgr.batches()
    meas = [torch.zeros((1, 7, b.size), dtype=b.torch_dtype(), device="cuda") for b in bs]
    for t in meas:
        t[:, 6] = 1.0
    has = [torch.zeros((1, b.size), dtype=torch.uint8, device="cuda") for b in bs]
    deltas = [torch.full((b.size,), float("nan"), dtype=torch.float64, device="cuda") for b in bs]
    poses = [torch.full((b.size, 7), float("nan"), dtype=torch.float64, device="cuda") for b in bs]
    rows = [_slots(b, ids) for b, ids in zip(bs, idss)]
    out = [(np.full(cs.n, np.nan), np.full((cs.n, 7), np.nan)) for _ in bs]
    for k, (origin, radius) in enumerate(cs.scenes):
        mgr.step_sequence_all(0.0, meas, has_meas=has, query=(origin, radius, deltas, poses), use_graph=use_graph)
        torch.cuda.synchronize()
        sel = cs.scene == k
        for j in range(len(bs)):
            out[j][0][sel], out[j][1][sel] = deltas[j].cpu().numpy()[rows[j]][sel], poses[j].cpu().numpy()[rows[j]][sel]
    _assert_state(mgr, cs, idss[0])
    return out


def _live(mgr, cs, ids):
    """The resident kernels with the per-tick query: one session of one predict-only tick per scene (idle limits as tests/test_gpu_live.py)"""
    bs = mgr.batches()
    meas = [torch.zeros((1, 7, b.size), dtype=b.torch_dtype(), device="cuda") for b in bs]
    has = [torch.zeros((1, b.size), dtype=torch.uint8, device="cuda") for b in bs]
    deltas = [torch.full((b.size,), float("nan"), dtype=torch.float64, device="cuda") for b in bs]
    poses = [torch.full((b.size, 7), float("nan"), dtype=torch.float64, device="cuda") for b in bs]
    rows = _slots(bs[0], ids)

    def q(origin, radius):
        torch.cuda.synchronize()
        mgr.live_start_all(0.0, meas, has_meas=has, max_ticks=1, idle_limit_s=3.0, query=(origin, radius, deltas, poses))
        mgr.live_post_all(1, one_doorbell_per_tick=True)
        assert mgr.live_wait_all(1, 5.0) and mgr.live_stop_all() == 1
        torch.cuda.synchronize()
        return deltas[0].cpu().numpy()[rows], poses[0].cpu().numpy()[rows]
    out = _per_scene(cs, q)
    _assert_state(mgr, cs, ids)
    return out


# ---- the cases (also run by the child process, see _all_cases) ---------------------------------------------------------------------

def _case_standalone(models, dtype):
    """1 and 3: the standalone kernel at own time -- held to the rule -- and at t1 = t0, the indexed launch with the ids in random
    order, the scalar entries: the same bits.  Returns the standalone answers."""
    cs = cases(dtype)
    mgr, ids = _create(models, cs)
    b = mgr.batches()[0]
    rows = _slots(b, ids)
    want = _standalone(mgr, cs, ids)
    assert np.array_equal(want[1][:, 3:], np.tile(IDENT, (cs.n, 1)))
    accept("intersect_kernel", models, cs, want[0], want[1][:, :3])

    def at_t0(origin, radius):
        d, p = b.intersect_sphere(origin, radius, t1=0.0)
        return d.cpu().numpy()[rows], p.cpu().numpy()[rows]
    _same("intersect_sphere at t1 = t0", _per_scene(cs, at_t0), want)
    perm = np.random.default_rng(17).permutation(cs.n)

    def indexed(origin, radius):
        d, p, found = mgr.intersect_batch(ids[perm], 0.0, origin, radius)
        assert found.all()
        out = np.empty(cs.n), np.empty((cs.n, 7))
        out[0][perm], out[1][perm] = d, p
        return out
    _same("intersect_batch, random order", _per_scene(cs, indexed), want)
    rng = np.random.default_rng(19)
    some = [int(rng.choice(np.nonzero(cs.family == f)[0])) for f in range(len(cs.family_names)) for _ in range(3)]
    some += [int(i) for i in np.nonzero(~cs.clear)[0][:3]]
    for i in some:
        origin, radius = cs.scenes[cs.scene[i]]
        ok, p7, d = mgr.intersection_pose(int(ids[i]), 0.0, origin, radius)
        assert d == want[0][i] and np.array_equal(p7, want[1][i]) and ok == bool(d > -1), i
        assert mgr.intersection_time(int(ids[i]), 0.0, origin, radius) == want[0][i], i
    mgr.close()
    return want


def _case_neighbours(models, want):
    """2: created grouped by family (the fixture's order: whole wavefronts settled by Sturm's chain) and interleaved"""
    cs = cases("f64")
    order = _interleaved(cs)
    assert len(set(cs.family[order[:64]].tolist())) >= 8
    mgr, ids = _create(models, cs, order=order)
    _same("interleaved families", _standalone(mgr, cs, ids), want)
    mgr.close()


def _case_other_models(models, want):
    """4: angular_rates inlines the same solver -- the same delta, bit for bit, and a position that passes the rule; the models
    without an acceleration answer -1"""
    cs = cases("f64")
    mgr, ids = _create(models, cs, "angular_rates")
    d, p = _standalone(mgr, cs, ids)
    assert np.array_equal(d, want[0])
    q = p[:, 3:] * np.sign(p[:, 6:7])
    assert np.abs(q - IDENT).max() <= 1e-15
    accept("intersect_kernel, angular_rates", models, cs, d, p[:, :3])
    mgr.close()
    for name in ("uniform_velocity", "angular_velocities"):
        m = models[name]
        mgr = te.TargetManager(dtype="f64")
        ids = np.arange(cs.n, dtype=np.uint32)
        assert mgr.init_batch(ids, DT, 0.0, pose6(cs.p)[0], pose6(cs.v)[1], pose6(cs.a)[1], type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == cs.n
        d, p = mgr.batches()[0].intersect_sphere(*cs.scenes[0])
        assert (d.cpu().numpy() == -1).all() and np.array_equal(p.cpu().numpy(), np.tile([0, 0, 0] + IDENT, (cs.n, 1)))
        mgr.close()


def _case_fused(models, want, what):
    """5: the fused queries.  Predict-only ticks with dt = 0 keep p, v, a to the bit (asserted in _fused)."""
    from test_gpu_parity import coupled
    cs = cases("f64")
    m = models["uniform_acceleration"]
    kw, mats, layout, shared = dict(shared_axes=False), None, "axis_separable_packed", 0
    if what in ("separable, shared axes", "population, shared axes"):
        kw, shared = dict(shared_axes=True), 1
    elif what == "dense, 3 lanes":
        kw, layout = dict(lanes_per_target=3), None
    elif what == "dense, coupled matrices":
        kw, mats, layout = {}, coupled(m), "symmetric_packed"
    mgr, ids = _create(models, cs, mats=mats, order=_interleaved(cs), **kw)
    idss, wants = [ids], [want]
    if what.startswith("population"):     # a second batch of the other model with a quartic to solve: one launch per tick for both
        _, ids2 = _create(models, cs, "angular_rates", mgr=mgr, first_id=50_000)
        assert mgr.population_tick() and len(mgr.batches()) == 2 and mgr.batches()[1].shared_axes == shared
        idss.append(ids2)
        wants.append(_standalone(mgr, cs, ids2, 1))                  # (the standalone kernel on that batch, before any tick)
        assert np.array_equal(wants[1][0], want[0])
    b = mgr.batches()[0]
    assert layout is None or b.layout == layout, b.layout
    assert b.shared_axes == shared and (what != "dense, 3 lanes" or b.lanes_per_target == 3)
    if what == "resident":
        _same("resident kernel", _live(mgr, cs, ids), want)
    else:
        for use_graph in (0, 1):
            for got, w, model in zip(_fused(mgr, cs, idss, use_graph), wants, ("uniform_acceleration", "angular_rates")):
                _same("%s, %s, %s" % (what, "recorded" if use_graph else "eager", model), got, w)
    mgr.close()


FUSED = ["separable, shared axes", "separable, plain", "dense, 3 lanes", "dense, coupled matrices", "population", "population, shared axes",
         "resident"]


def _all_cases():
    """Entry point of the child process (policies forced by the environment, see the module docstring): items 1 and 5."""
    assert os.environ.get("TE_PINGPONG_MIN_MB") == "0" and os.environ.get("TE_ZIGZAG_MIN_MB") == "0"
    models = _models()
    want = _case_standalone(models, "f64")
    for what in FUSED:
        _case_fused(models, want, what)
    print("quartic cases ok")


# ---- tests ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def standalone(models):
    return _case_standalone(models, "f64")


def test_standalone_kernel_f64(standalone):
    pass


def test_standalone_kernel_f32_state(models):
    _case_standalone(models, "f32")


def test_neighbours_do_not_matter(models, standalone):
    _case_neighbours(models, standalone)


def test_other_models_inline_the_same_solver(models, standalone):
    _case_other_models(models, standalone)


@pytest.mark.parametrize("what", FUSED)
def test_fused_queries_give_the_standalone_bits(models, standalone, what):
    _case_fused(models, standalone, what)


def test_forced_ab_ticks_and_zigzag():
    env = dict(os.environ, TE_PINGPONG_MIN_MB="0", TE_ZIGZAG_MIN_MB="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_quartic_cases as t; t._all_cases()"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "quartic cases ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
