"""The target clock at 250 Hz over long uptimes: every path that advances or reads a target's time, against exact time.

The reference keeps one double per target, t_ = t0 and t_ = t_ + dt on every update (target_interface.cpp:28,151); the
getters at t1 extrapolate by t1 - t_.  Here a target's time is t_base[slot] + t_acc (the batch clock plus a per-slot offset,
te_clock.hpp).  At dt = 0.004 (no exact binary form), after hours of uptime and for targets created while the node runs,
no sum of times is exact, so each check holds the library's clock to the reference's own drift:

    |t_lib - t_exact| <= 8 |t_ref - t_exact| + 2 ulp(t_exact)

t_exact = Fraction(t0) + the sum of the Fraction(dt) actually passed; t_ref = the sequential double sum from t0, as the
reference computes it; ulp of the target's own time.  Read through target_manager_get_time (Batch::time) and, in the
oracle scenario, through everything that extrapolates to t1: the f80 oracle is handed the exact offset t1 - t_exact rounded
once, so a clock error of the library shows up as an output error under test_gpu_precision's K / CEIL rule.
`pytest -s` prints the worst |t_lib - t_exact| / max(|t_ref - t_exact|, ulp) of every path."""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import oracle
from conftest import synth_stream
from test_highprec_kat import f32r

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

from test_gpu_precision import CEIL, ORIGIN, RADIUS, _ix_margin, _row, _unsign, check_query  # noqa: E402

DT = {"250Hz": 0.004, "60Hz": 1.0 / 60.0, "exact": 2.0 ** -8}
EPOCH = 1.7e9                      # ROS time: seconds since 1970
DAY_DT, DAY_TICKS = 8640.0123, 10  # brings a batch clock to ~86 400 s in ten predict-only ticks
TWO_MODELS = ("uniform_acceleration", "angular_rates")
WORST = {}


class Clock:
    """Exact and reference time of one target (or of a group that is always updated together)."""

    def __init__(self, t0):
        self.exact, self.ref = Fraction(t0), float(t0)

    def tick(self, dt, n=1):
        self.exact += n * Fraction(dt)
        r = self.ref
        for _ in range(n):
            r += dt
        self.ref = r


def check_clock(path, tag, t_lib, clk):
    e_lib = abs(Fraction(t_lib) - clk.exact)
    e_ref = abs(Fraction(clk.ref) - clk.exact)
    u = Fraction(math.ulp(float(clk.exact)))
    ratio = float(e_lib / max(e_ref, u))
    WORST[path] = max(WORST.get(path, 0.0), ratio)
    assert e_lib <= 8 * e_ref + 2 * u, (
        "%s %s: |t_lib - t_exact| = %.3e s > 8 x |t_ref - t_exact| (%.3e s) + 2 ulp (%.1e s); t_exact %.17g t_lib %.17g t_ref %.17g"
        % (path, tag, e_lib, e_ref, u, float(clk.exact), t_lib, clk.ref))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[clock] worst |t_lib - t_exact| / max(|t_ref - t_exact|, ulp(t)) per path:")
    for k in sorted(WORST):
        print("[clock]   %-40s %8.3f" % (k, WORST[k]))


def _p0(n, seed):
    rng = np.random.default_rng(seed)
    p0 = np.zeros((n, 7))
    p0[:, :3] = rng.uniform(-10, 10, (n, 3))
    p0[:, 6] = 1.0
    return p0


def _init(mgr, models, name, ids, dt, t0, seed):
    m = models[name]
    assert mgr.init_batch(ids, dt, t0, _p0(len(ids), seed), type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"]) == len(ids)


def _ring(b, ticks=1):
    """a measurement ring of `ticks` identical ticks (the targets' initial positions) in the batch's precision"""
    n = b.size
    meas = np.zeros((ticks, 7, n))
    meas[:, 6, :] = 1.0
    return torch.from_numpy(meas).to("cuda").to(b.torch_dtype()).contiguous()


def _check_all(mgr, path, tag, clocks):
    for tid, clk in clocks.items():
        check_clock(path, "%s id %d" % (tag, tid), mgr.getTime(tid), clk)


# ---- a. batch ticks only: t0 = 0 and t0 = 1e5 in the same batches, 1e5 ticks on each path ---------------------------------------
PATHS = ("step_dense", "sequence_eager_1000", "graph_1", "graph_1000", "fused_1000", "population_1000", "live")
A_CASES = [(p, "f64", "250Hz", 100000) for p in PATHS] + [(p, "f32", "60Hz", 100000) for p in PATHS] + \
          [(p, "f64", "exact", 10000) for p in PATHS]


def _advance(mgr, path, dt, ticks):
    bs = mgr.batches()
    if path == "step_dense":
        for b in bs:
            for _ in range(ticks):
                b.step(dt)
    elif path == "graph_1":
        for b in bs:
            r = _ring(b)
            for _ in range(ticks):
                b.step_sequence(dt, r, use_graph=True)
    elif path in ("sequence_eager_1000", "graph_1000"):
        for b in bs:
            r = _ring(b)
            for _ in range(ticks // 1000):
                b.step_sequence(dt, r, use_graph=path == "graph_1000", n_ticks=1000)
    elif path == "fused_1000":
        for b in bs:
            r = _ring(b, 1000)
            for _ in range(ticks // 1000):
                b.step_fused(dt, r)
    elif path == "population_1000":
        assert mgr.population_tick()
        rings = [_ring(b) for b in bs]
        for _ in range(ticks // 1000):
            mgr.step_sequence_all(dt, rings, use_graph=True, n_ticks=1000)
    elif path == "live":
        rings = [_ring(b) for b in bs]
        torch.cuda.synchronize()
        mgr.live_start_all(dt, rings, max_ticks=ticks, idle_limit_s=5.0)
        mgr.live_post_all(ticks)
        assert mgr.live_wait_all(ticks, 60.0)
        assert mgr.live_stop_all() == ticks
    else:
        raise AssertionError(path)


@pytest.mark.parametrize("path,dtype,rate,ticks", A_CASES)
def test_batch_ticks(models, path, dtype, rate, ticks):
    dt = DT[rate]
    mgr = te.TargetManager(dtype=dtype)
    clocks = {}
    for k, name in enumerate(TWO_MODELS):
        for t0 in (0.0, 1e5):
            ids = np.arange(3, dtype=np.uint32) + 100 * k + (10 if t0 else 0)
            _init(mgr, models, name, ids, dt, t0, seed=int(ids[0]))
            clocks.update({int(i): Clock(t0) for i in ids})
    assert len(mgr.batches()) == 2
    _advance(mgr, path, dt, ticks)
    for clk in clocks.values():
        clk.tick(dt, ticks)
    _check_all(mgr, "%s %s %s" % (path, dtype, rate), "after %d ticks" % ticks, clocks)
    if rate == "exact":   # every sum is exact: so is the library's clock
        for tid, clk in clocks.items():
            assert mgr.getTime(tid) == clk.exact
    mgr.close()


# ---- b. born late: the batch clock at ~86 400 s, targets created at 0, at the clock and at ROS epoch time, driven by id --------------
def _day_old_manager(models, dtype, names=TWO_MODELS):
    """A manager whose batches (one per model) have run a day: a filler target per batch, ten predict-only ticks of
    DAY_DT, then erased (a batch tick on an empty batch does not move its clock).  Returns the manager and the clock."""
    mgr = te.TargetManager(dtype=dtype)
    fillers = []
    for k, name in enumerate(names):
        fid = 900000 + k
        _init(mgr, models, name, np.array([fid], dtype=np.uint32), DAY_DT, 0.0, seed=fid)
        fillers.append(fid)
    for b in mgr.batches():
        for _ in range(DAY_TICKS):
            b.step(DAY_DT)
    day = Clock(0.0)
    day.tick(DAY_DT, DAY_TICKS)
    for fid in fillers:
        check_clock("born_late filler", "id %d" % fid, mgr.getTime(fid), day)
    clock = mgr.getTime(fillers[0])
    for fid in fillers:
        assert mgr.erase(fid)
    return mgr, clock


def _born_late_targets(mgr, models, n, dt, clock, first_id=1000):
    """n targets over the two models and t0 = 0, the batch clock, EPOCH (any three of them cover the three times);
    returns {id: Clock}"""
    combos = [(TWO_MODELS[j % 2], t0) for j, t0 in enumerate((0.0, clock, EPOCH, 0.0, clock, EPOCH))]
    clocks = {}
    for j, (name, t0) in enumerate(combos):
        cnt = n // 6 + (1 if j < n % 6 else 0)
        if cnt == 0:
            continue
        ids = np.arange(cnt, dtype=np.uint32) + first_id + 1000 * j
        _init(mgr, models, name, ids, dt, t0, seed=int(ids[0]))
        clocks.update({int(i): Clock(t0) for i in ids})
    return clocks


def _drive_by_id(mgr, clocks, dt, ticks, per_call, scalar=False, every=1000):
    """every tick: each target updated by id (calls naming per_call ids, or the scalar C ABI one id at a time); every
    `every` ticks one batch-wide tick as well"""
    ids = np.array(sorted(clocks), dtype=np.uint32)
    meas = np.tile([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], (len(ids), 1))
    parts = [ids[i:i + per_call] for i in range(0, len(ids), per_call)]
    one = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    for s in range(ticks):
        if scalar:
            for tid in ids:
                mgr.update(int(tid), dt, one)
        else:
            for p in parts:
                mgr.update_batch(p, dt, meas[:len(p)])
        if s % every == every - 1:
            if scalar:
                mgr.update_all(dt)
            else:
                for b in mgr.batches():
                    b.step(dt)
    for clk in clocks.values():   # every update adds the same dt: the order of by-id and batch-wide ones does not matter
        clk.tick(dt, ticks + ticks // every)


def born_late_case(models, dtype, rate, per_call, ticks, scalar=False):
    dt = DT[rate]
    path = "born_late %s%s" % ("scalar ABI" if scalar else "by id x%d" % per_call, "" if os.environ.get("TE_SMALL_BATCH_QUEUE", "1") != "0" else " (bulk)")
    mgr, clock = _day_old_manager(models, dtype)
    clocks = _born_late_targets(mgr, models, per_call if per_call > 1 else 3, dt, clock)
    _check_all(mgr, path, "%s %s at creation" % (dtype, rate), clocks)
    _drive_by_id(mgr, clocks, dt, ticks, per_call, scalar=scalar)
    _check_all(mgr, path, "%s %s after %d ticks" % (dtype, rate, ticks), clocks)
    if rate == "exact":
        for tid, clk in clocks.items():
            assert mgr.getTime(tid) == clk.exact, tid
    mgr.close()


@pytest.mark.parametrize("dtype,rate,per_call,ticks",
                         [("f64", "250Hz", 1, 100000), ("f32", "250Hz", 1, 20000), ("f64", "60Hz", 1, 20000),
                          ("f64", "250Hz", 40, 20000), ("f32", "60Hz", 40, 20000), ("f64", "exact", 40, 10000),
                          ("f64", "250Hz", 300, 20000), ("f32", "250Hz", 300, 10000)])
def test_born_late_by_id(models, dtype, rate, per_call, ticks):
    born_late_case(models, dtype, rate, per_call, ticks)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_born_late_scalar_c_abi(models, dtype):
    born_late_case(models, dtype, "250Hz", 1, 10000, scalar=True)


def _bulk_case():
    """(child process, TE_SMALL_BATCH_QUEUE=0) the born-late scenario through the staged bulk path of the by-id calls"""
    import conftest
    models = {k: oracle.load_model_yaml(conftest.model_path(k)) for k in conftest.MODEL_FILES}
    born_late_case(models, "f64", "250Hz", 40, 10000)
    born_late_case(models, "f32", "60Hz", 300, 5000)
    print("WORST " + json.dumps(WORST))
    print("bulk clock ok")


def test_born_late_bulk_path():
    env = dict(os.environ, TE_SMALL_BATCH_QUEUE="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_clock as t; t._bulk_case()"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "bulk clock ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    for line in p.stdout.splitlines():
        if line.startswith("WORST "):
            for k, v in json.loads(line[6:]).items():
                WORST[k] = max(WORST.get(k, 0.0), v)


# ---- c. slot churn: erase (swap with the last slot), batched erase (compaction), re-creation into reused slots --------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_time_travels_with_the_target(models, dtype):
    dt = DT["250Hz"]
    rng = np.random.default_rng(7)
    mgr, clock = _day_old_manager(models, dtype)
    clocks = _born_late_targets(mgr, models, 12, dt, clock)
    next_id = 50000
    one = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    for rnd in range(30):
        ids = np.array(sorted(clocks), dtype=np.uint32)
        for _ in range(150):                      # random subsets by id: every target ends up with its own count of updates
            sub = ids[rng.random(len(ids)) < 0.5]
            if len(sub):
                mgr.update_batch(sub, dt, np.tile(one, (len(sub), 1)))
                for tid in sub:
                    clocks[int(tid)].tick(dt)
        for b in mgr.batches():                   # a batch-wide tick
            b.step(dt)
        for clk in clocks.values():
            clk.tick(dt)
        victim = int(ids[rng.integers(len(ids) // 2)])       # one erase: the last slot of its batch moves into the hole
        assert mgr.erase(victim)
        del clocks[victim]
        ids = np.array(sorted(clocks), dtype=np.uint32)
        gone = rng.choice(ids, 3, replace=False)              # a batched erase: survivors from the tail fill the holes
        assert mgr.erase_batch(gone) == 3
        for g in gone:
            del clocks[int(g)]
        for k, name in enumerate(TWO_MODELS):                 # new targets into the freed slots
            t0 = (0.0, EPOCH + rnd, 5e4 + 0.1 * rnd)[rnd % 3]
            new = np.arange(2, dtype=np.uint32) + next_id
            next_id += 2
            _init(mgr, models, name, new, dt, t0, seed=int(new[0]))
            clocks.update({int(i): Clock(t0) for i in new})
        _check_all(mgr, "slot churn %s" % dtype, "round %d" % rnd, clocks)
    mgr.close()


# ---- d. what reads the clock: getters at t1, intersections at t1, the gated query, the log -- against the f80 oracle -------------
def _meas_stream(name, n, ticks, dt, seed, dtype):
    p0, meas = synth_stream(name, n, ticks, seed=seed, dt=dt)
    rd = f32r if dtype == "f32" else (lambda a: np.array(a, dtype=np.float64))
    return rd(p0), rd(meas)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_outputs_at_t1_against_the_oracle(models, dtype, tmp_path):
    """Targets born at t0 = 0 and at EPOCH after a day of batch clock, 4000 ticks by id with measurements (a batch-wide
    predict-only tick every 500), then every reader of the clock at a t1 that is not the target's own time."""
    dt, ticks, n = DT["250Hz"], 4000, 8
    rd = f32r if dtype == "f32" else (lambda a: np.array(a, dtype=np.float64))
    mgr, clock = _day_old_manager(models, dtype)
    cases = []
    for k, name in enumerate(TWO_MODELS):
        m = models[name]
        p0, meas = _meas_stream(name, n, ticks, dt, 500 + k, dtype)
        ids = np.arange(n, dtype=np.uint32) + 2000 + 100 * k
        Q, R, P0 = rd(m["Q"]), rd(m["R"]), rd(m["P"])
        groups = [(ids[: n // 2], 0.0), (ids[n // 2:], EPOCH)]
        for g, t0 in groups:
            sel = np.isin(ids, g)
            assert mgr.init_batch(g, dt, t0, p0[sel], type=m["model"], Q=Q, R=R, P0=P0) == len(g)
        orcs = {d: oracle.OracleBatch(m["model"], Q, R, P0, p0, dt, 0.0, dtype=d) for d in (dtype, "f80")}
        cases.append(dict(name=name, ids=ids, meas=meas, orcs=orcs, groups=[(g, t0, Clock(t0)) for g, t0 in groups]))
    all_ids = np.concatenate([c["ids"] for c in cases])
    for s in range(ticks):
        meas = np.concatenate([c["meas"][s] for c in cases])
        mgr.update_batch(all_ids, dt, meas)
        for c in cases:
            for o in c["orcs"].values():
                o.step(dt, c["meas"][s])
        if s % 500 == 499:
            for b in mgr.batches():
                b.step(dt)
            for c in cases:
                for o in c["orcs"].values():
                    o.step(dt)
    for c in cases:
        for _, _, clk in c["groups"]:
            clk.tick(dt, ticks + ticks // 500)
    path = "oracle scenario %s" % dtype
    mgr.set_log_directory(tmp_path)
    mgr.set_log_targets(all_ids)
    mgr.log()
    for c in cases:
        name, ceil = c["name"], CEIL[dtype][c["name"]]
        inp = dict(dtype=dtype, name=name)
        for g, t0, clk in c["groups"]:
            rows = np.nonzero(np.isin(c["ids"], g))[0]
            for tid in g:
                t_lib = mgr.getTime(int(tid))
                check_clock(path, "id %d" % tid, t_lib, clk)
                with open(os.path.join(tmp_path, "time_%d" % tid)) as f:     # the log's time channel (%g)
                    assert float(f.read().split()[-1]) == float("%g" % t_lib)
            own = float(clk.exact)
            for t1 in (own, own + 0.1, own + 1.0):
                q = float(Fraction(t1) - clk.exact)          # the exact offset, rounded once
                ref = {}
                for d, o in c["orcs"].items():
                    o.set_times(0.0)
                    ref[d] = np.concatenate([o.pose_at(q), o.twist_at(q), o.acceleration_at(q)], 1)[rows]
                p, tw, ac, found = mgr.get_est_batch(g, t1=t1)
                assert found.all()
                got = np.concatenate([p, tw, ac], 1)
                got[:, 3:7] = _unsign(got[:, 3:7], ref["f80"][:, 3:7])
                same = ref[dtype].copy()
                same[:, 3:7] = _unsign(same[:, 3:7], ref["f80"][:, 3:7])
                tag = "%s t0=%g get_est_batch at own%+g" % (name, t0, t1 - own)
                _row(tag, dtype, "out", got, same, ref["f80"], ceil["out"])
            t1 = own + 0.1
            q = float(Fraction(t1) - clk.exact)
            ix = {d: o.intersection_pose(q, ORIGIN, RADIUS) for d, o in c["orcs"].items()}
            ref = {d: dict(ix=(ix[d][2][rows], ix[d][1][rows])) for d in ix}
            ref["margin"] = _ix_margin(c["orcs"]["f80"], q)[rows]
            delta, pose, found = mgr.intersect_batch(g, t1, ORIGIN, RADIUS)
            assert found.all()
            check_query("%s t0=%g intersect_batch at own+0.1" % (name, t0), inp, ref, delta, pose, min_hits=0)
            one = [mgr.intersection_pose(int(tid), t1, ORIGIN, RADIUS) for tid in g]
            check_query("%s t0=%g intersection_pose at own+0.1" % (name, t0), inp, ref, np.array([r[2] for r in one]),
                        np.array([r[1] for r in one]), min_hits=0)
            conv, pose_c, delta_c, _ = mgr.intersect_converged_batch(g, t1, 1e-3, 1e-3, ORIGIN, RADIUS)
            check_query("%s t0=%g intersect_converged_batch at own+0.1" % (name, t0), inp, ref, delta_c, pose_c, min_hits=0)
    mgr.close()
