"""The shared-axes storage form of the separable layout with packed groups (csrc/te_layout.hpp LAYOUT_SEPARABLE_SHARED): an
fp64 batch whose x, y, z chains (and roll, pitch, yaw chains of angular_rates) have equal Q blocks, R entries and P0 blocks
stores and steps ONE covariance block per kind of axis.  It must give the bits of the plain form.

Every comparison here is np.array_equal between two managers of ONE process on the same seeded stream: a plain one
(shared_axes=False) and a shared one -- x and the full P from get_state_batch, pose / twist / acceleration from get_est_batch.
The first test checks the premise itself on the plain manager alone: after 200 masked ticks the blocks of one kind are the same
bits on every axis, in the GPU's own code.

The cases run twice: in the pytest process with the default policies, and in a child process with TE_PINGPONG_MIN_MB=0 and
TE_ZIGZAG_MIN_MB=0 (read once per process), where every eager tick without the fused query is an A -> B tick and consecutive
ticks walk the tiles -- of a batch, and of a whole population launch -- in opposite directions."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MODEL_FILES, model_path

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

NAMES = ["angular_rates", "angular_velocities", "uniform_acceleration", "uniform_velocity"]
RECORD_WORDS = {"angular_rates": 33, "angular_velocities": 39, "uniform_acceleration": 15, "uniform_velocity": 9}
PLAIN_WORDS = {"angular_rates": 57, "angular_velocities": 45, "uniform_acceleration": 27, "uniform_velocity": 15}
ALGORITHMIC_BYTES = {"angular_rates": 584, "angular_velocities": 680, "uniform_acceleration": 264, "uniform_velocity": 168}
DT = 0.004


def _models():
    import oracle
    return {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}


def _kinds(name):
    """[(axes of the kind, row stride between the states of a chain, states per chain)]"""
    if name == "angular_rates":
        return [((0, 1, 2), 6, 3), ((3, 4, 5), 6, 3)]
    if name == "angular_velocities":
        return [((0, 1, 2), 6, 2)]
    return [((0, 1, 2), 3, 3 if name == "uniform_acceleration" else 2)]


def _block(P, axis, stride, nb):
    rows = [axis + stride * b for b in range(nb)]
    return P[:, rows][:, :, rows]


def _manager(shared):
    mgr = te.TargetManager(dtype="f64", shared_axes=shared)
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    return mgr


def _create(mgr, m, name, ids, p0, Q=None, P0=None):
    n = len(ids)
    assert mgr.init_batch(ids, DT, 0.0, p0, type=te.MODEL_TYPES[name], Q=m["Q"] if Q is None else Q, R=m["R"],
                          P0=m["P"] if P0 is None else P0) == n


def _state(mgr, ids):
    torch.cuda.synchronize()
    x, P = mgr.get_state_batch(ids)
    pose, twist, acc, found = mgr.get_est_batch(ids)
    assert found.all() and np.isfinite(x).all() and np.isfinite(P).all()
    return x, P, pose, twist, acc


def _assert_same(plain, shared, ids, what):
    a, b = _state(plain, ids), _state(shared, ids)
    for u, v, part in zip(a, b, ("x", "P", "pose", "twist", "acceleration")):
        assert np.array_equal(u, v), "%s: %s differs, max |d| = %g" % (what, part, np.abs(u - v).max())


def _pair(models, name, n, seed, ticks, availability=1.0):
    from target_estimation_amd.streams import make_stream
    st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, seed, availability=availability)
    ids = np.arange(n, dtype=np.uint32) + 1000
    p0 = st["p0"].cpu().numpy()
    plain, shared = _manager(False), _manager(True)
    for mgr in (plain, shared):
        _create(mgr, models[name], name, ids, p0)
    pb, sb = plain.batches()[0], shared.batches()[0]
    assert pb.shared_axes == 0 and sb.shared_axes == 1
    assert (pb.layout, pb.lanes_per_target) == (sb.layout, sb.lanes_per_target) == ("axis_separable_packed", 1)
    return plain, shared, pb, sb, ids, st


# ---- the cases (also run by the child process, see _all_cases) -------------------------------------------------------

def _case_premise_and_long_masked_run(models, name):
    """200 ticks, 90 % availability, a ragged last tile.  First the premise, on the plain manager alone."""
    n, ticks = 64 * 5 + 17, 200
    plain, shared, pb, sb, ids, st = _pair(models, name, n, 41, ticks, availability=0.9)
    assert st["has_meas"] is not None and 0.85 < float(st["has_meas"].float().mean()) < 0.95
    pb.step_sequence(DT, st["meas"], st["has_meas"])
    _, P, _, _, _ = _state(plain, ids)
    for axes, stride, nb in _kinds(name):
        first = _block(P, axes[0], stride, nb)
        assert np.abs(first).max() > 0
        for ax in axes[1:]:
            assert np.array_equal(first, _block(P, ax, stride, nb)), "%s: axis %d's block is not axis %d's" % (name, ax, axes[0])
    if name == "angular_rates":
        assert not np.array_equal(_block(P, 0, 6, 3), _block(P, 3, 6, 3))   # (different kinds do differ)
    sb.step_sequence(DT, st["meas"], st["has_meas"])
    _assert_same(plain, shared, ids, name + " masked run")
    assert pb.shared_axes == 0 and sb.shared_axes == 1
    plain.close(); shared.close()


def _case_by_id_erase_query_pose(models, name):
    """By-id updates in random order (the queued one-target path and the indexed launch), erase and re-create, the fused own-time
    sphere query, the per-tick pose stream, recorded and eager sequences."""
    n, ticks = 64 * 20 + 17, 12
    plain, shared, pb, sb, ids, st = _pair(models, name, n, 43, ticks, availability=0.9)
    rng = np.random.default_rng(5)
    meas_rows = st["meas"].permute(0, 2, 1).cpu().numpy()     # [ticks, n, 7]
    has = st["has_meas"].cpu().numpy()
    for mgr, b in ((plain, pb), (shared, sb)):
        r = np.random.default_rng(6)
        b.step_sequence(DT, st["meas"][:4], st["has_meas"][:4], use_graph=True)
        order = r.permutation(n)                               # every target, random order: an indexed launch
        assert mgr.update_batch(ids[order], DT, meas_rows[4][order], has[4][order]) == n
        some = r.permutation(n)[:200]                          # a few: the one-target queue
        assert mgr.update_batch(ids[some], DT, meas_rows[5][some], has[5][some]) == 200
        mgr.update_batch(ids[some[:50]], DT)                   # predict only
        for i in some[:5]:
            mgr.update(int(ids[i]), DT, meas_rows[6][i])
    _assert_same(plain, shared, ids, name + " by id")
    gone = np.sort(1 + rng.permutation(n - 1)[:70])
    p_new = meas_rows[7][gone]
    for mgr in (plain, shared):
        assert mgr.erase_batch(ids[gone]) == 70
        mgr.erase(int(ids[0]))                                 # (one target: the single-move path)
        _create(mgr, models[name], name, ids[gone], p_new)     # the same ids again: new targets in the freed slots' place
    live = ids[1:]
    _assert_same(plain, shared, live, name + " erase / re-create")
    out = []
    for mgr, b in ((plain, pb), (shared, sb)):
        sz = b.size
        order = [int(i) - 1000 for i in b.slot_ids()]          # slot -> column of the stream
        m = st["meas"][8:12][:, :, order].contiguous()
        h = st["has_meas"][8:12][:, order].contiguous()
        delta = torch.full((sz,), float("nan"), dtype=torch.float64, device="cuda")
        qpose = torch.full((sz, 7), float("nan"), dtype=torch.float64, device="cuda")
        poses = torch.full((2, 7, sz), float("nan"), dtype=torch.float64, device="cuda")
        mgr.step_sequence_all(DT, [m[:1]], has_meas=[h[:1]], query=([0.0, 0.0, 0.0], 50.0, [delta], [qpose]), use_graph=0)
        b.step_sequence(DT, m[1:3], h[1:3], poses=poses)       # POSE
        mgr.step_sequence_all(DT, [m[3:]], has_meas=[h[3:]], query=([0.0, 0.0, 0.0], 50.0, [delta], [qpose]), use_graph=1,
                              poses=[poses[:1]])               # POSE + QUERY, recorded
        torch.cuda.synchronize()
        out.append((b.slot_ids(), delta.cpu().numpy(), qpose.cpu().numpy(), poses.cpu().numpy()))
    for u, v, part in zip(out[0], out[1], ("slot ids", "query delta", "query pose", "pose stream")):
        assert np.array_equal(u, v, equal_nan=False), name + ": " + part
    _assert_same(plain, shared, live, name + " query / pose ticks")
    assert pb.shared_axes == 0 and sb.shared_axes == 1
    plain.close(); shared.close()


def _case_population(models):
    """All four models in one manager: the one-launch population tick, eager and recorded, a mask on one batch, with the fused
    query and with pose streams."""
    from target_estimation_amd.streams import make_stream
    parts = [("angular_rates", 64 * 9 + 3), ("angular_velocities", 517), ("uniform_acceleration", 40), ("uniform_velocity", 64 * 12 + 50)]
    ticks = 10
    sts = [make_stream(te.MODEL_TYPES[nm], n, ticks, DT, 70 + k, availability=0.9 if k == 1 else 1.0) for k, (nm, n) in enumerate(parts)]
    plain, shared = _manager(False), _manager(True)
    all_ids = []
    for mgr in (plain, shared):
        base = 0
        for (nm, n), st in zip(parts, sts):
            ids = np.arange(n, dtype=np.uint32) + base
            base += 100_000
            _create(mgr, models[nm], nm, ids, st["p0"].cpu().numpy())
            if mgr is plain:
                all_ids.append(ids)
        assert mgr.population_tick()
    assert [b.shared_axes for b in plain.batches()] == [0] * 4 and [b.shared_axes for b in shared.batches()] == [1] * 4
    meas = [st["meas"] for st in sts]
    has = [st["has_meas"] for st in sts]
    out = []
    for mgr in (plain, shared):
        sz = [b.size for b in mgr.batches()]
        delta = [torch.full((s,), float("nan"), dtype=torch.float64, device="cuda") for s in sz]
        qpose = [torch.full((s, 7), float("nan"), dtype=torch.float64, device="cuda") for s in sz]
        poses = [torch.full((2, 7, s), float("nan"), dtype=torch.float64, device="cuda") for s in sz]
        cut = lambda a, b: ([m[a:b] for m in meas], [None if h is None else h[a:b] for h in has])   # noqa: E731
        m, h = cut(0, 3)
        mgr.step_sequence_all(DT, m, has_meas=h, use_graph=0)                      # eager, three ticks: both directions when zig-zag is on
        m, h = cut(3, 5)
        mgr.step_sequence_all(DT, m, has_meas=h, use_graph=1)                      # recorded
        m, h = cut(5, 6)
        mgr.step_sequence_all(DT, m, has_meas=h, query=([0.0, 0.0, 0.0], 50.0, delta, qpose), use_graph=0)
        m, h = cut(6, 8)
        mgr.step_sequence_all(DT, m, has_meas=h, use_graph=0, poses=poses)         # pose streams, eager
        m, h = cut(8, 10)
        mgr.step_sequence_all(DT, m, has_meas=h, query=([0.0, 0.0, 0.0], 50.0, delta, qpose), use_graph=1, poses=[poses[0], None, poses[2], None])
        torch.cuda.synchronize()
        assert mgr.population_tick()
        out.append([t.cpu().numpy() for t in delta + qpose + poses])
    for u, v in zip(out[0], out[1]):
        assert np.array_equal(u, v)
    for ids, (nm, _) in zip(all_ids, parts):
        _assert_same(plain, shared, ids, "population tick, " + nm)
    plain.close(); shared.close()


def _all_cases():
    """Entry point of the child process (policies forced by the environment, see the module docstring)."""
    assert os.environ.get("TE_PINGPONG_MIN_MB") == "0" and os.environ.get("TE_ZIGZAG_MIN_MB") == "0"
    models = _models()
    for name in NAMES:
        _case_premise_and_long_masked_run(models, name)
        _case_by_id_erase_query_pose(models, name)
    _case_population(models)
    print("shared axes cases ok")


# ---- tests ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_blocks_of_one_kind_are_bit_equal_then_shared_equals_plain(models, name):
    _case_premise_and_long_masked_run(models, name)


@pytest.mark.parametrize("name", NAMES)
def test_by_id_erase_recreate_query_and_pose(models, name):
    _case_by_id_erase_query_pose(models, name)


def test_population_tick(models):
    _case_population(models)


def test_all_cases_with_forced_ab_ticks_and_zigzag():
    env = dict(os.environ, TE_PINGPONG_MIN_MB="0", TE_ZIGZAG_MIN_MB="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_shared_axes as t; t._all_cases()"], env=env, capture_output=True, text=True,
                       timeout=1200)
    assert p.returncode == 0 and "shared axes cases ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


@pytest.mark.parametrize("name", NAMES)
def test_sizes(models, name):
    one = np.tile([0, 0, 0, 0, 0, 0, 1.0], (70, 1))
    ids = np.arange(70, dtype=np.uint32)
    plain, shared, single = _manager(False), _manager(True), te.TargetManager(dtype="f32", shared_axes=True)
    for mgr in (plain, shared, single):
        _create(mgr, models[name], name, ids, one)
    pb, sb, fb = plain.batches()[0], shared.batches()[0], single.batches()[0]
    assert (sb.shared_axes, sb.record_words, sb.algorithmic_bytes) == (1, RECORD_WORDS[name], ALGORITHMIC_BYTES[name])
    assert (pb.shared_axes, pb.record_words) == (0, PLAIN_WORDS[name])
    assert pb.algorithmic_bytes == ALGORITHMIC_BYTES[name] + 2 * 8 * (PLAIN_WORDS[name] - RECORD_WORDS[name])
    assert sb.resident_bytes_per_target == RECORD_WORDS[name] * 8 and pb.resident_bytes_per_target == PLAIN_WORDS[name] * 8
    assert (fb.shared_axes, fb.record_words) == (0, PLAIN_WORDS[name])            # fp32 batches are never shared
    assert sb.live_capacity == pb.live_capacity and sb.shared_axes == 1            # (answers for the plain form, without leaving the shared one)
    assert shared._lib.target_manager_set_shared_axes(shared._h, 0) != 0 and sb.shared_axes == 1   # refused once a batch exists
    for mgr in (plain, shared, single):
        mgr.close()


@pytest.mark.parametrize("name", NAMES)
def test_ineligible_matrices_stay_plain(models, name):
    """One axis' Q block scaled by (1 + 2^-52); one target whose own P0 has a different y block: never shared, today's results."""
    from target_estimation_amd.streams import make_stream
    m = models[name]
    n, ticks = 200, 12
    st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, 91)
    ids = np.arange(n, dtype=np.uint32)
    p0 = st["p0"].cpu().numpy()
    axes, stride, nb = _kinds(name)[0]
    rows = [axes[1] + stride * b for b in range(nb)]
    Q2 = np.array(m["Q"], dtype=np.float64).copy()
    Q2[np.ix_(rows, rows)] *= 1.0 + 2.0 ** -52
    assert not np.array_equal(Q2, m["Q"])
    P2 = np.tile(np.asarray(m["P"], dtype=np.float64), (n, 1, 1))
    P2[7][np.ix_(rows, rows)] *= 1.5
    for kw in (dict(Q=Q2), dict(P0=P2)):
        plain, shared = _manager(False), _manager(True)
        for mgr in (plain, shared):
            _create(mgr, m, name, ids, p0, **kw)
            assert mgr.batches()[0].shared_axes == 0 and mgr.batches()[0].record_words == PLAIN_WORDS[name]
            mgr.batches()[0].step_sequence(DT, st["meas"])
        _assert_same(plain, shared, ids, name + " ineligible " + next(iter(kw)))
        plain.close(); shared.close()


@pytest.mark.parametrize("what", ["step_fused", "live_start", "second_class", "other_p0", "init_batch_classes"])
@pytest.mark.parametrize("name", NAMES)
def test_demotion_continues_bit_equal(models, name, what):
    """A shared batch that has ticked meets something the shared form does not serve: it is expanded to the plain records and goes
    on as a manager that was never shared."""
    from target_estimation_amd.streams import make_stream
    m = models[name]
    n, ticks = 64 * 3 + 9, 14
    st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, 93)
    ids = np.arange(n, dtype=np.uint32)
    p0 = st["p0"].cpu().numpy()
    more = np.arange(40, dtype=np.uint32) + 5000
    axes, stride, nb = _kinds(name)[0]
    rows = [axes[2] + stride * b for b in range(nb)]
    plain, shared = _manager(False), _manager(True)
    wide = torch.zeros((ticks, 7, n + 40), dtype=torch.float64, device="cuda")
    wide[:, 6, :] = 1.0
    wide[:, :, :n] = st["meas"]
    for mgr in (plain, shared):
        _create(mgr, m, name, ids, p0)
        b = mgr.batches()[0]
        assert b.shared_axes == (1 if mgr is shared else 0)
        b.step_sequence(DT, st["meas"][:5])
        if what == "step_fused":
            b.step_fused(DT, st["meas"][5:8])
        elif what == "live_start":
            assert b.live_capacity >= n
            b.live_start(DT, st["meas"][5:8].contiguous(), max_ticks=3, idle_limit_s=3.0)
            b.live_post(3)
            assert b.live_wait(3, 5.0) and b.live_stop() == 3
        elif what == "second_class":
            mgr.init_batch(more, DT, 5 * DT, p0[:40], type=te.MODEL_TYPES[name], Q=2.0 * np.asarray(m["Q"]), R=m["R"], P0=m["P"])
        elif what == "other_p0":
            P2 = np.asarray(m["P"], dtype=np.float64).copy()
            P2[np.ix_(rows, rows)] *= 3.0
            mgr.init_batch(more, DT, 5 * DT, p0[:40], type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=P2)
        else:
            Qs = np.stack([np.asarray(m["Q"]), 2.0 * np.asarray(m["Q"])])
            Rs = np.stack([np.asarray(m["R"])] * 2)
            Ps = np.stack([np.asarray(m["P"])] * 2)
            mgr.init_batch_classes(more, DT, 5 * DT, p0[:40], te.MODEL_TYPES[name], Qs, Rs, Ps, np.arange(40) % 2)
        assert len(mgr.batches()) == 1 and b.shared_axes == 0 and b.record_words == PLAIN_WORDS[name]
        b.step_sequence(DT, (wide if b.size > n else st["meas"])[8:])
    _assert_same(plain, shared, ids, "%s after %s" % (name, what))
    if plain.batches()[0].size > n:
        _assert_same(plain, shared, more, "%s after %s, the new targets" % (name, what))
    plain.close(); shared.close()


def test_switch_in_the_environment():
    """TE_SHARED_AXES=0 keeps every batch plain; the per-manager setter still turns the form on for one manager."""
    code = ("import numpy as np, target_estimation_amd as te, sys, os\n"
            "sys.path.insert(0, %r)\n"
            "from conftest import model_path\n"
            "ids = np.arange(70, dtype=np.uint32)\n"
            "one = np.tile([0, 0, 0, 0, 0, 0, 1.0], (70, 1))\n"
            "a = te.TargetManager(model_path('angular_rates')); a.init_batch(ids, 0.004, 0.0, one)\n"
            "b = te.TargetManager(model_path('angular_rates'), shared_axes=True); b.init_batch(ids, 0.004, 0.0, one)\n"
            "print('forms', a.batches()[0].shared_axes, b.batches()[0].shared_axes)\n" % os.path.dirname(__file__))
    for value, want in (("0", "forms 0 1"), ("1", "forms 1 1")):
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TE_SHARED_AXES=value), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and want in p.stdout, p.stdout[-1000:] + p.stderr[-2000:]
