"""The reversed tick's block order (csrc/zigzag_map.hpp zz_block: the workgroups mirrored inside each class b % 8) must step
every tile exactly once, whatever the grid: a tile stepped twice, or not at all, changes its targets' state.

The cases run in a child process with TE_ZIGZAG_MIN_MB=0 (read once per process), where consecutive dense ticks of every batch
-- and of a whole population launch -- walk the workgroups in opposite directions: once with the default small-grid policy (one
wavefront per workgroup: block = wavefront) and once with TE_SMALL_GRID_WAVES=0 (four wavefronts per workgroup).  The pytest
process steps the same cases with the default policies, i.e. forwards on every tick (these batches are far below the 128 MB
at which a batch zig-zags), and every target's x and P from get_state_batch must be the same bits.  Every target has its own
measurements (streams.make_stream), so no two tiles hold the same state.

Single batches: grids of 1, 7, 8, 9, 17 and 23 workgroups with a ragged last tile, every motion model in fp64 (shared-axes form)
and fp32 (plain form), plus angular_rates fp64 with coupled matrices on 3 lanes per target (the dense kernel on the upper
triangle, G > 1); six eager ticks -- three of them reversed -- then the same block of measurements recorded and replayed.
Population launches: parts of (3, 5), (8, 1) and (9, 7, 2) workgroups with a ragged part in the middle, eager and recorded,
both precisions."""
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
GRIDS = (1, 7, 8, 9, 17, 23)
POPULATIONS = ((3, 5), (8, 1), (9, 7, 2))
DT = 0.004
TICKS = 6


def _models():
    import oracle
    return {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}


def _manager(dtype, **kw):
    mgr = te.TargetManager(dtype=dtype, shared_axes=(dtype == "f64"), **kw)
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    return mgr


def _state(mgr, ids):
    torch.cuda.synchronize()
    x, P = mgr.get_state_batch(ids)
    assert np.isfinite(x).all() and np.isfinite(P).all()
    return x, P


def _single(models, name, dtype, n, seed, mats=None, lanes=0):
    from target_estimation_amd.streams import make_stream
    m = models[name] if mats is None else mats
    st = make_stream(te.MODEL_TYPES[name], n, TICKS, DT, seed, dtype=dtype)
    ids = np.arange(n, dtype=np.uint32) + 1000
    mgr = _manager(dtype, lanes_per_target=lanes)
    assert mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
    b = mgr.batches()[0]
    if lanes:
        assert b.lanes_per_target == lanes % 100 and b.layout == "symmetric_packed"
    else:
        assert b.layout == "axis_separable_packed" and b.shared_axes == (1 if dtype == "f64" else 0)
    b.step_sequence(DT, st["meas"], use_graph=False)   # six eager ticks: forwards, backwards, ...
    b.step_sequence(DT, st["meas"], use_graph=True)    # the same block, recorded (a recording starts forwards)
    out = _state(mgr, ids)
    mgr.close()
    return out


def _population(models, dtype, blocks, wpb, seed):
    from target_estimation_amd.streams import make_stream
    ragged = 5 if wpb == 1 else 70   # (wpb == 4: the last workgroup of the part has an empty wavefront and a ragged one)
    cut = 1 if len(blocks) > 2 else 0   # the ragged part: its last tile lies inside the grid, not at its end
    sizes = [k * wpb * 64 - (ragged if i == cut else 0) for i, k in enumerate(blocks)]
    mgr = _manager(dtype)
    sts, all_ids = [], []
    for i, (name, n) in enumerate(zip(NAMES, sizes)):   # (the order of the parts in the grid: angular_rates first)
        st = make_stream(te.MODEL_TYPES[name], n, TICKS, DT, seed + i, dtype=dtype)
        ids = np.arange(n, dtype=np.uint32) + 100_000 * i
        m = models[name]
        assert mgr.init_batch(ids, DT, 0.0, st["p0"].cpu().numpy(), type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
        sts.append(st)
        all_ids.append(ids)
    assert mgr.population_tick() and [b.size for b in mgr.batches()] == sizes
    meas = [st["meas"] for st in sts]
    mgr.step_sequence_all(DT, meas, use_graph=0)
    mgr.step_sequence_all(DT, meas, use_graph=1)
    assert mgr.population_tick()
    out = [a for ids in all_ids for a in _state(mgr, ids)]
    mgr.close()
    return out


def _run_cases(wpb):
    """{case: arrays}; wpb = wavefronts per workgroup of the launches in the child process (it sizes the batches)."""
    from test_gpu_parity import coupled
    models = _models()
    out = {}
    seed = 500
    for blocks in GRIDS:
        n = blocks * wpb * 64 - 5
        for name in NAMES:
            for dtype in ("f64", "f32"):
                seed += 1
                x, P = _single(models, name, dtype, n, seed)
                out["%s_%s_%d_x" % (name, dtype, blocks)], out["%s_%s_%d_P" % (name, dtype, blocks)] = x, P
    # the dense kernel on 3 lanes per target: 21 targets per wavefront
    x, P = _single(models, "angular_rates", "f64", 17 * wpb * 21 - 5, 900, mats=coupled(models["angular_rates"]), lanes=103)
    out["dense_G3_x"], out["dense_G3_P"] = x, P
    for blocks in POPULATIONS:
        for dtype in ("f64", "f32"):
            seed += 10
            for k, a in enumerate(_population(models, dtype, blocks, wpb, seed)):
                out["population_%s_%s_%d" % ("_".join(map(str, blocks)), dtype, k)] = a
    return out


def _child(wpb, path):
    """Entry point of the child process: every tick that can be reversed is."""
    assert os.environ.get("TE_ZIGZAG_MIN_MB") == "0"
    assert os.environ.get("TE_SMALL_GRID_WAVES") == ("0" if wpb == 4 else None)
    np.savez(path, **_run_cases(wpb))
    print("zigzag cases ok")


@pytest.mark.parametrize("wpb", [1, 4])
def test_reversed_ticks_equal_forward_ticks_bit_for_bit(tmp_path, wpb):
    assert "TE_ZIGZAG_MIN_MB" not in os.environ and "TE_SMALL_GRID_WAVES" not in os.environ   # this process steps forwards
    path = str(tmp_path / "zigzag.npz")
    env = dict(os.environ, TE_ZIGZAG_MIN_MB="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    if wpb == 4:
        env["TE_SMALL_GRID_WAVES"] = "0"
    p = subprocess.run([sys.executable, "-c", "import test_gpu_zigzag_affine as t; t._child(%d, %r)" % (wpb, path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "zigzag cases ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    forwards = _run_cases(wpb)
    with np.load(path) as zigzag:
        assert sorted(zigzag.files) == sorted(forwards)
        differ = [k for k in sorted(forwards) if not np.array_equal(forwards[k], zigzag[k])]
    assert not differ, "reversed ticks changed the state of: " + ", ".join(differ)
