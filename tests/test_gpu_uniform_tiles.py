"""Uniform tiles of the shared-axes storage form (csrc/te_layout.hpp Cfg::UT, csrc/batch_store.hpp): a tile whose 64 targets hold
the same bits in their linear-chain covariance words keeps ONE copy of them, and its dense tick neither reads nor writes the record
chunks that hold only such words.  It must give the bits of a manager without the feature.

Every comparison is np.array_equal of get_state_batch plus get_est_batch between two managers of ONE process on one seeded
stream, uniform_tiles=False and uniform_tiles=True (both in the shared-axes form).  The cases run twice: in the pytest process, and
in a child process with TE_PINGPONG_MIN_MB=0 TE_ZIGZAG_MIN_MB=0 (A -> B ticks, reversed tile walks), as tests/test_gpu_shared_axes.py.

Shapes: 64 * 3 + 17 = 209 targets per model (three full tiles and a ragged one); the population case uses four ragged sizes.

The angular_velocities kernels are built without the feature (te_layout.hpp uniform_tiles_model: they sit at the register limit
of three wavefronts per SIMD and two of their 85 words would be skippable): its batches never flag a tile and report the form's
constant figures, and its cases check exactly that next to the bits."""
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
FULL_BYTES = {"angular_rates": 584, "angular_velocities": 680, "uniform_acceleration": 264, "uniform_velocity": 168}
# words of a tile's block / record chunks a uniform tile skips (te_layout.hpp Cfg::LW, LIN_CHUNKS); 0: built without the feature
BLOCK_WORDS = {"angular_rates": 12, "angular_velocities": 0, "uniform_acceleration": 6, "uniform_velocity": 3}
SKIPPED_CHUNKS = {"angular_rates": 6, "angular_velocities": 0, "uniform_acceleration": 3, "uniform_velocity": 1}
PROMOTE_AFTER = 2      # dense ticks since the last settle before a tick looks for uniform tiles (Batch::promote_after)
DT = 0.004
N = 64 * 3 + 17


def _models():
    import oracle
    return {k: oracle.load_model_yaml(model_path(k)) for k in MODEL_FILES}


def _tiles(n):
    return (n + 63) // 64


def _expect(name, k):
    """flagged tiles expected of a batch of this model where a batch with the feature has k"""
    return k if BLOCK_WORDS[name] else 0


def _bytes(name, n, flagged):
    """the documented figure (include/target_estimation_amd/target_batch_c.h): `flagged` = the flagged tiles' indices"""
    in_them = sum(min(64, n - 64 * t) for t in flagged)
    total = n * FULL_BYTES[name] - in_them * 2 * 16 * SKIPPED_CHUNKS[name] + len(flagged) * (2 * 8 * BLOCK_WORDS[name] + 4)
    return total // n


def _manager(on, dtype="f64", **kw):
    mgr = te.TargetManager(dtype=dtype, uniform_tiles=on, **kw)
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    return mgr


def _create(mgr, m, name, ids, p0, t0=0.0, **kw):
    assert mgr.init_batch(ids, DT, t0, p0, type=te.MODEL_TYPES[name], Q=kw.get("Q", m["Q"]), R=m["R"], P0=m["P"]) == len(ids)


def _state(mgr, ids):
    torch.cuda.synchronize()
    x, P = mgr.get_state_batch(ids)
    pose, twist, acc, found = mgr.get_est_batch(ids)
    assert found.all() and np.isfinite(x).all() and np.isfinite(P).all()
    return x, P, pose, twist, acc


def _assert_same(off, on, ids, what):
    a, b = _state(off, ids), _state(on, ids)
    for u, v, part in zip(a, b, ("x", "P", "pose", "twist", "acceleration")):
        assert np.array_equal(u, v), "%s: %s differs, max |d| = %g" % (what, part, np.abs(u - v).max())


def _pair(models, name, n, seed, ticks, availability=1.0):
    from target_estimation_amd.streams import make_stream
    st = make_stream(te.MODEL_TYPES[name], n, ticks, DT, seed, availability=availability)
    ids = np.arange(n, dtype=np.uint32) + 1000
    p0 = st["p0"].cpu().numpy()
    off, on = _manager(False), _manager(True)
    for mgr in (off, on):
        _create(mgr, models[name], name, ids, p0)
    fb, nb = off.batches()[0], on.batches()[0]
    assert fb.shared_axes == 1 and nb.shared_axes == 1
    assert fb.uniform_tiles == 0 and nb.uniform_tiles == 0
    assert fb.algorithmic_bytes == nb.algorithmic_bytes == FULL_BYTES[name]      # before the first tick: the form's constant
    return off, on, fb, nb, ids, st


def _promote(pairs, st, first):
    """PROMOTE_AFTER + 1 unmasked dense ticks, meas ticks first .. on every (manager's) batch"""
    for b in pairs:
        for s in range(PROMOTE_AFTER + 1):
            b.step(DT, st["meas"][first + s])
    return first + PROMOTE_AFTER + 1


# ---- the cases (also run by the child process, see _all_cases) -------------------------------------------------------

def _case_unmasked(models, name):
    """30 ticks, a different dt every tick; the state read back every tick (which must not change the count)."""
    off, on, fb, nb, ids, st = _pair(models, name, N, 11, 30)
    all_tiles = list(range(_tiles(N)))
    for s in range(30):
        dt = DT * (1.0 + 0.37 * ((s * 7) % 5))
        for b in (fb, nb):
            b.step(dt, st["meas"][s])
        _assert_same(off, on, ids, "%s unmasked tick %d" % (name, s))
        want = _expect(name, len(all_tiles)) if s + 1 >= PROMOTE_AFTER + 1 else 0      # the ragged tile included
        assert nb.uniform_tiles == want and fb.uniform_tiles == 0, (name, s, nb.uniform_tiles, want)
        assert fb.algorithmic_bytes == FULL_BYTES[name]
        if want:
            assert nb.algorithmic_bytes == _bytes(name, N, all_tiles) < FULL_BYTES[name]
        else:
            assert nb.algorithmic_bytes == FULL_BYTES[name]
    off.close(); on.close()


def _case_masks(models, name):
    off, on, fb, nb, ids, st = _pair(models, name, N, 13, 60, availability=0.9)
    T = _tiles(N)
    s = _promote((fb, nb), st, 0)
    assert nb.uniform_tiles == _expect(name, T)
    zero = torch.zeros(N, dtype=torch.uint8, device="cuda")
    for b in (fb, nb):
        b.step(DT, st["meas"][s], zero)                       # every target missed: the tiles stay uniform
    s += 1
    _assert_same(off, on, ids, name + " all-zero mask")
    assert nb.uniform_tiles == _expect(name, T)
    split = torch.ones(N, dtype=torch.uint8, device="cuda")
    split[64 + 6] = 0                                         # one lane of tile 1 misses its measurement
    for b in (fb, nb):
        b.step(DT, st["meas"][s], split)
    s += 1
    _assert_same(off, on, ids, name + " one tile split")
    assert nb.uniform_tiles == _expect(name, T - 1)
    assert nb.algorithmic_bytes == (_bytes(name, N, [0, 2, 3]) if BLOCK_WORDS[name] else FULL_BYTES[name])
    for k in range(4):                                        # its lanes differ now: it stays out
        for b in (fb, nb):
            b.step(DT, st["meas"][s])
        s += 1
        _assert_same(off, on, ids, name + " after the split, tick %d" % k)
        assert nb.uniform_tiles == _expect(name, T - 1)
    for k in range(40):                                       # 90 % random masks
        for b in (fb, nb):
            b.step(DT, st["meas"][s], st["has_meas"][s])
        s += 1
        _assert_same(off, on, ids, name + " random mask, tick %d" % k)
    assert fb.uniform_tiles == 0
    off.close(); on.close()


def _case_touching_records(models, name):
    """By-id updates, erase / re-create and a second init_batch between dense ticks."""
    off, on, fb, nb, ids, st = _pair(models, name, N, 17, 40)
    T = _tiles(N)
    rows = st["meas"].permute(0, 2, 1).cpu().numpy()          # [ticks, n, 7]
    s = _promote((fb, nb), st, 0)
    assert nb.uniform_tiles == _expect(name, T)
    # the indexed launch over every target, all measured: the count goes to 0 and every tile comes back behind the gate
    order = np.random.default_rng(3).permutation(N)
    for mgr in (off, on):
        assert mgr.update_batch(ids[order], DT, rows[s][order], np.ones(N, dtype=np.uint8)) == N
    s += 1
    assert nb.uniform_tiles == 0
    _assert_same(off, on, ids, name + " indexed launch")
    for k in range(PROMOTE_AFTER + 1):
        assert nb.uniform_tiles == 0
        for b in (fb, nb):
            b.step(DT, st["meas"][s])
        s += 1
    assert nb.uniform_tiles == _expect(name, T)
    _assert_same(off, on, ids, name + " re-promoted")
    # the one-target queue with a per-entry dt, on targets of tile 0 only: tile 0 stays out
    for mgr in (off, on):
        mgr.update(int(ids[3]), DT, rows[s][3])
        mgr.update(int(ids[9]), 2.5 * DT, rows[s][9])
        mgr.update(int(ids[11]), 0.5 * DT)                    # predict only
    s += 1
    assert nb.uniform_tiles == 0
    for b in (fb, nb):
        for k in range(PROMOTE_AFTER + 1):
            b.step(DT, st["meas"][s + k])
    s += PROMOTE_AFTER + 1
    assert nb.uniform_tiles == _expect(name, T - 1)
    assert nb.algorithmic_bytes == (_bytes(name, N, [1, 2, 3]) if BLOCK_WORDS[name] else FULL_BYTES[name])
    _assert_same(off, on, ids, name + " one-target queue")
    # the queue with one dt for all (no per-entry dt), tile 2
    for mgr in (off, on):
        assert mgr.update_batch(ids[[130, 140]], DT, rows[s][[130, 140]]) == 2
    s += 1
    assert nb.uniform_tiles == 0
    for b in (fb, nb):
        for k in range(PROMOTE_AFTER + 1):
            b.step(DT, st["meas"][s + k])
    s += PROMOTE_AFTER + 1
    assert nb.uniform_tiles == _expect(name, T - 2)
    _assert_same(off, on, ids, name + " queue, one dt")
    # erase five targets of tile 1 (survivors from the ragged tile -- bit-uniform with it -- fill the holes), re-create them:
    # the new targets land in the ragged tile, whose lanes then differ
    gone = ids[64:69]
    for mgr, b in ((off, fb), (on, nb)):
        assert mgr.erase_batch(gone) == 5
        _create(mgr, models[name], name, gone, rows[s][64:69], t0=0.0)
    assert nb.uniform_tiles == 0 and nb.size == N
    cols = [int(i) - 1000 for i in nb.slot_ids()]
    assert cols == [int(i) - 1000 for i in fb.slot_ids()]
    for b in (fb, nb):
        for k in range(PROMOTE_AFTER + 1):
            b.step(DT, st["meas"][s + k][:, cols].contiguous())
    s += PROMOTE_AFTER + 1
    assert nb.uniform_tiles == _expect(name, 1)               # tile 1 alone: 0 and 2 were touched above, 3 holds the new targets
    _assert_same(off, on, ids, name + " erase / re-create")
    # a second init_batch appended into the ragged tile after promotion
    more = np.arange(10, dtype=np.uint32) + 9000
    wide = torch.zeros((7, N + 10), dtype=torch.float64, device="cuda")
    wide[6] = 1.0
    for mgr in (off, on):
        _create(mgr, models[name], name, more, rows[s][:10], t0=0.0)
    assert nb.uniform_tiles == 0 and nb.size == N + 10
    for b in (fb, nb):
        for k in range(PROMOTE_AFTER + 1):
            wide[:, :N] = st["meas"][s + k][:, cols]
            b.step(DT, wide)
    assert nb.uniform_tiles == _expect(name, 1)
    _assert_same(off, on, np.concatenate([ids, more]), name + " second init_batch")
    assert fb.uniform_tiles == 0
    off.close(); on.close()


def _case_emptied_batch(models, name):
    """A batch emptied by erases that move no record (the whole batch at once, then the last slot one by one) and filled again:
    the flags of the targets that left must not describe the new ones."""
    off, on, fb, nb, ids, st = _pair(models, name, 64 + 6, 31, 2 * (PROMOTE_AFTER + 1) + 4)
    rows = st["meas"].permute(0, 2, 1).cpu().numpy()
    s = _promote((fb, nb), st, 0)
    assert nb.uniform_tiles == _expect(name, 2)
    for mgr in (off, on):
        assert mgr.erase_batch(ids) == len(ids)
    assert nb.size == 0 and nb.uniform_tiles == 0
    few = ids[:40]
    for mgr in (off, on):
        _create(mgr, models[name], name, few, rows[s][:40], t0=0.0)
    assert nb.uniform_tiles == 0 and nb.algorithmic_bytes == FULL_BYTES[name]
    for k in range(2):                                        # below the gate: no tile may be flagged, or taken for flagged
        for b in (fb, nb):
            b.step(DT, st["meas"][s][:, :40].contiguous())
        s += 1
        assert nb.uniform_tiles == 0
        _assert_same(off, on, few, "%s emptied and filled again, tick %d" % (name, k))
    for k in range(PROMOTE_AFTER + 1):
        for b in (fb, nb):
            b.step(DT, st["meas"][s][:, :40].contiguous())
        s += 1
    assert nb.uniform_tiles == _expect(name, 1)
    for mgr in (off, on):
        for i in few[::-1]:                                   # always the last slot
            assert mgr.erase(int(i))
        _create(mgr, models[name], name, few[:9], rows[s][:9], t0=0.0)
    assert nb.uniform_tiles == 0
    for b in (fb, nb):
        b.step(DT, st["meas"][s + 1][:, :9].contiguous())
    _assert_same(off, on, few[:9], name + " emptied slot by slot and filled again")
    off.close(); on.close()


def _case_launch_variants(models, name):
    """The fused sphere query, the per-tick pose stream, recorded and eager sequences, step_sequence_all with and without graphs."""
    off, on, fb, nb, ids, st = _pair(models, name, N, 19, 24, availability=0.9)
    T = _tiles(N)
    out = []
    for mgr, b in ((off, fb), (on, nb)):
        m, h = st["meas"], st["has_meas"]
        delta = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        qpose = torch.full((N, 7), float("nan"), dtype=torch.float64, device="cuda")
        poses = torch.full((2, 7, N), float("nan"), dtype=torch.float64, device="cuda")
        q = ([0.0, 0.0, 0.0], 50.0, [delta], [qpose])
        b.step_sequence(DT, m[0:2], use_graph=True)           # recorded: promotes from its first tick
        assert b.uniform_tiles == (_expect(name, T) if b is nb else 0)
        b.step_sequence(DT, m[2:5])                           # eager
        mgr.step_sequence_all(DT, [m[5:6]], query=q, use_graph=0)                  # QUERY
        b.step_sequence(DT, m[6:8], poses=poses)                                   # POSE
        mgr.step_sequence_all(DT, [m[8:10]], query=q, use_graph=1, poses=[poses])  # POSE + QUERY, recorded
        assert b.uniform_tiles == (_expect(name, T) if b is nb else 0)
        mgr.step_sequence_all(DT, [m[10:12]], has_meas=[h[10:12]], use_graph=1)    # masks, recorded
        mgr.step_sequence_all(DT, [m[12:16]], has_meas=[h[12:16]], query=q, use_graph=0, poses=[poses])
        b.step_sequence(DT, m[16:20], h[16:20], use_graph=True)
        b.step_sequence(DT, m[20:24], use_graph=True)
        torch.cuda.synchronize()
        out.append((delta.cpu().numpy(), qpose.cpu().numpy(), poses.cpu().numpy()))
    for u, v, part in zip(out[0], out[1], ("query delta", "query pose", "pose stream")):
        assert np.array_equal(u, v), name + ": " + part
    _assert_same(off, on, ids, name + " launch variants")
    off.close(); on.close()


def _case_population(models):
    """All four models in one manager, four ragged sizes: the one-launch population tick, eager and recorded, with a mask on one
    batch, the fused query and pose streams."""
    from target_estimation_amd.streams import make_stream
    parts = [("angular_rates", 64 * 3 + 17), ("angular_velocities", 64 * 2 + 5), ("uniform_acceleration", 40), ("uniform_velocity", 64 * 4 + 50)]
    ticks = 14
    sts = [make_stream(te.MODEL_TYPES[nm], n, ticks, DT, 70 + k, availability=0.9 if k == 3 else 1.0) for k, (nm, n) in enumerate(parts)]
    off, on = _manager(False), _manager(True)
    all_ids = []
    for mgr in (off, on):
        base = 0
        for (nm, n), st in zip(parts, sts):
            ids = np.arange(n, dtype=np.uint32) + base
            base += 100_000
            _create(mgr, models[nm], nm, ids, st["p0"].cpu().numpy())
            if mgr is off:
                all_ids.append(ids)
        assert mgr.population_tick()
    meas = [st["meas"] for st in sts]
    has = [st["has_meas"] for st in sts]
    out = []
    for mgr in (off, on):
        sz = [b.size for b in mgr.batches()]
        delta = [torch.full((s,), float("nan"), dtype=torch.float64, device="cuda") for s in sz]
        qpose = [torch.full((s, 7), float("nan"), dtype=torch.float64, device="cuda") for s in sz]
        poses = [torch.full((2, 7, s), float("nan"), dtype=torch.float64, device="cuda") for s in sz]
        q = ([0.0, 0.0, 0.0], 50.0, delta, qpose)
        cut = lambda a, b: [m[a:b] for m in meas]             # noqa: E731
        mgr.step_sequence_all(DT, cut(0, 4), use_graph=0)                          # eager, unmasked: promotes at its third tick
        counts = [b.uniform_tiles for b in mgr.batches()]
        assert counts == ([_expect(nm, _tiles(n)) for nm, n in parts] if mgr is on else [0] * 4), counts
        if mgr is on:
            for b, (nm, n) in zip(mgr.batches(), parts):
                assert b.algorithmic_bytes == (_bytes(nm, n, range(_tiles(n))) if BLOCK_WORDS[nm] else FULL_BYTES[nm])
        mgr.step_sequence_all(DT, cut(4, 6), has_meas=[None, None, None, has[3][4:6]], use_graph=0)   # a mask on one batch
        mgr.step_sequence_all(DT, cut(6, 8), use_graph=1)                          # recorded
        mgr.step_sequence_all(DT, cut(8, 9), query=q, use_graph=0)
        mgr.step_sequence_all(DT, cut(9, 11), use_graph=0, poses=poses)
        mgr.step_sequence_all(DT, cut(11, 13), query=q, use_graph=1, poses=[poses[0], None, poses[2], None])
        mgr.step_sequence_all(DT, cut(13, 14), has_meas=[None, None, None, has[3][13:14]], use_graph=1)
        torch.cuda.synchronize()
        assert mgr.population_tick()
        out.append([t.cpu().numpy() for t in delta + qpose + poses])
    for u, v in zip(out[0], out[1]):
        assert np.array_equal(u, v)
    for ids, (nm, _) in zip(all_ids, parts):
        _assert_same(off, on, ids, "population tick, " + nm)
    assert [b.uniform_tiles for b in off.batches()] == [0] * 4
    off.close(); on.close()


def _case_demotion(models, name, what):
    """A batch with flagged tiles meets something the shared form does not serve: settled, expanded, and bit-equal from there."""
    off, on, fb, nb, ids, st = _pair(models, name, N, 23, 14)
    T = _tiles(N)
    _promote((fb, nb), st, 0)
    assert nb.uniform_tiles == _expect(name, T)
    more = np.arange(20, dtype=np.uint32) + 7000
    wide = torch.zeros((14, 7, N + 20), dtype=torch.float64, device="cuda")
    wide[:, 6, :] = 1.0
    wide[:, :, :N] = st["meas"]
    for mgr, b in ((off, fb), (on, nb)):
        if what == "step_fused":
            b.step_fused(DT, st["meas"][3:6])
        elif what == "live_start":
            assert b.live_capacity >= N
            b.live_start(DT, st["meas"][3:6].contiguous(), max_ticks=3, idle_limit_s=3.0)
            b.live_post(3)
            assert b.live_wait(3, 5.0) and b.live_stop() == 3
        else:
            m = models[name]
            mgr.init_batch(more, DT, 3 * DT, st["p0"].cpu().numpy()[:20], type=te.MODEL_TYPES[name], Q=2.0 * np.asarray(m["Q"]), R=m["R"], P0=m["P"])
        assert b.shared_axes == 0 and b.uniform_tiles == 0
        b.step_sequence(DT, (wide if b.size > N else st["meas"])[6:])
        assert b.uniform_tiles == 0
    _assert_same(off, on, ids, "%s after %s" % (name, what))
    off.close(); on.close()


def _case_other_batches(models, name):
    """fp32, plain-form and per-class batches: never a flagged tile, today's figures."""
    from target_estimation_amd.streams import make_stream
    m = models[name]
    ids = np.arange(N, dtype=np.uint32)
    st64 = make_stream(te.MODEL_TYPES[name], N, 6, DT, 29)
    st32 = make_stream(te.MODEL_TYPES[name], N, 6, DT, 29, dtype="f32")
    single, plain, classes = _manager(True, dtype="f32"), _manager(True, shared_axes=False), _manager(True)
    for mgr, st in ((single, st32), (plain, st64)):
        _create(mgr, m, name, ids, st["p0"].cpu().numpy())
    Qs = np.stack([np.asarray(m["Q"]), 2.0 * np.asarray(m["Q"])])
    classes.init_batch_classes(ids, DT, 0.0, st64["p0"].cpu().numpy(), te.MODEL_TYPES[name], Qs, np.stack([np.asarray(m["R"])] * 2),
                               np.stack([np.asarray(m["P"])] * 2), np.arange(N) % 2)
    for mgr, st in ((single, st32), (plain, st64), (classes, st64)):
        b = mgr.batches()[0]
        assert b.shared_axes == 0
        before = b.algorithmic_bytes
        b.step_sequence(DT, st["meas"])
        b.step_sequence(DT, st["meas"][:4], use_graph=True)
        assert b.uniform_tiles == 0 and b.algorithmic_bytes == before
        mgr.close()


def _case_set_state(models, name):
    """Batch::set_state on a batch with flagged tiles, for the slots of tile 0 and a part of tile 1: every other target keeps
    its covariance (the blocks were written back before the batch left the shared form), and the pair goes on bit-equal.
    No public entry reaches Batch::set_state: the test build of the library has one (csrc/batch_store.cpp, TE_TEST_HOOKS)."""
    import ctypes
    assert te.capi.LIB.endswith("_testhooks.so")
    off, on, fb, nb, ids, st = _pair(models, name, N, 37, 10)
    T = _tiles(N)
    s = _promote((fb, nb), st, 0)
    assert nb.uniform_tiles == _expect(name, T)
    before = _state(off, ids)
    k = 64 + 6
    x = np.ascontiguousarray(before[0][:k] + 0.25)
    P = np.ascontiguousarray(before[1][:k] * 1.5)             # (exact, and it keeps the structure the layout stores)
    dp = ctypes.POINTER(ctypes.c_double)
    hook = fb._lib.te_test_batch_set_state
    hook.argtypes, hook.restype = [ctypes.c_void_p, ctypes.c_long, dp, dp], ctypes.c_int
    for b in (fb, nb):
        assert hook(b._h, k, x.ctypes.data_as(dp), P.ctypes.data_as(dp)) == 0
        assert b.shared_axes == 0 and b.uniform_tiles == 0
    for mgr in (off, on):
        got = _state(mgr, ids)
        assert np.array_equal(got[0][:k], x) and np.array_equal(got[1][:k], P)
        assert np.array_equal(got[0][k:], before[0][k:]) and np.array_equal(got[1][k:], before[1][k:])
    for b in (fb, nb):
        b.step_sequence(DT, st["meas"][s:])
        assert b.uniform_tiles == 0
    _assert_same(off, on, ids, name + " after set_state")
    off.close(); on.close()


def _set_state_cases():
    """Entry point of the child process that loads the test build of the library."""
    models = _models()
    for name in NAMES:
        _case_set_state(models, name)
    print("set_state cases ok")


def _all_cases():
    """Entry point of the child process (policies forced by the environment, see the module docstring)."""
    assert os.environ.get("TE_PINGPONG_MIN_MB") == "0" and os.environ.get("TE_ZIGZAG_MIN_MB") == "0"
    models = _models()
    for name in NAMES:
        _case_unmasked(models, name)
        _case_masks(models, name)
        _case_touching_records(models, name)
        _case_emptied_batch(models, name)
        _case_launch_variants(models, name)
        for what in ("step_fused", "live_start", "second_class"):
            _case_demotion(models, name, what)
        _case_other_batches(models, name)
    _case_population(models)
    print("uniform tiles cases ok")


# ---- tests ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_unmasked_run_flags_every_tile(models, name):
    _case_unmasked(models, name)


@pytest.mark.parametrize("name", NAMES)
def test_masks(models, name):
    _case_masks(models, name)


@pytest.mark.parametrize("name", NAMES)
def test_touching_records_between_dense_ticks(models, name):
    _case_touching_records(models, name)


@pytest.mark.parametrize("name", NAMES)
def test_batch_emptied_and_filled_again(models, name):
    _case_emptied_batch(models, name)


@pytest.mark.parametrize("name", NAMES)
def test_launch_variants(models, name):
    _case_launch_variants(models, name)


def test_population_tick(models):
    _case_population(models)


@pytest.mark.parametrize("what", ["step_fused", "live_start", "second_class"])
@pytest.mark.parametrize("name", NAMES)
def test_demotion_after_promotion(models, name, what):
    _case_demotion(models, name, what)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_plain_and_per_class_batches(models, name):
    _case_other_batches(models, name)


def test_set_state_after_promotion():
    from target_estimation_amd import _build
    lib = _build.build_testhooks()
    env = dict(os.environ, TARGET_ESTIMATION_AMD_LIB=lib,
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_uniform_tiles as t; t._set_state_cases()"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "set_state cases ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_switches():
    """TE_UNIFORM_TILES=0 in the environment; the setter is refused once a batch exists."""
    one = np.tile([0, 0, 0, 0, 0, 0, 1.0], (70, 1))
    ids = np.arange(70, dtype=np.uint32)
    mgr = te.TargetManager(model_path("angular_rates"))
    mgr.init_batch(ids, DT, 0.0, one)
    assert mgr._lib.target_manager_set_uniform_tiles(mgr._h, 0) != 0
    mgr.close()
    code = ("import numpy as np, torch, target_estimation_amd as te, sys\n"
            "sys.path.insert(0, %r)\n"
            "from conftest import model_path\n"
            "ids = np.arange(70, dtype=np.uint32)\n"
            "one = np.tile([0, 0, 0, 0, 0, 0, 1.0], (70, 1))\n"
            "m = torch.zeros((4, 7, 70), dtype=torch.float64, device='cuda'); m[:, 6] = 1.0\n"
            "out = []\n"
            "for kw in ({}, dict(uniform_tiles=True)):\n"
            "    a = te.TargetManager(model_path('angular_rates'), **kw); a.init_batch(ids, 0.004, 0.0, one)\n"
            "    b = a.batches()[0]; b.step_sequence(0.004, m); out.append(b.uniform_tiles)\n"
            "print('tiles', *out)\n" % os.path.dirname(__file__))
    for value, want in (("0", "tiles 0 2"), ("1", "tiles 2 2")):
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TE_UNIFORM_TILES=value), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and want in p.stdout, p.stdout[-1000:] + p.stderr[-2000:]


def test_all_cases_with_forced_ab_ticks_and_zigzag():
    env = dict(os.environ, TE_PINGPONG_MIN_MB="0", TE_ZIGZAG_MIN_MB="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_uniform_tiles as t; t._all_cases()"], env=env, capture_output=True, text=True,
                       timeout=1200)
    assert p.returncode == 0 and "uniform tiles cases ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
