"""The two caches of recorded sequences: a batch's (step_sequence(..., use_graph=True): 64 recordings, the least recently USED
one goes) and a manager's per device (step_sequence_all(..., use_graph=1): 8 recordings, the oldest one goes).  What is pinned:
which recording an eviction takes (through target_batch_graph_recordings) and that recording, evicting, recording again and
replaying leave the bits of the same ticks launched eagerly.  Every comparison is exact."""
import numpy as np
import pytest

from conftest import synth_stream
from test_gpu_parity import to_soa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

DT = 0.004


def _dts(k):
    """k distinct time steps"""
    return [DT * (1.0 + i / 128.0) for i in range(k)]


def _manager(models, parts, ticks, seed):
    mgr = te.TargetManager(dtype="f64")
    mgr.set_stream(torch.cuda.current_stream().cuda_stream)
    base, streams, ids = 0, [], []
    for k, (name, n) in enumerate(parts):
        m = models[name]
        p0, meas = synth_stream(name, n, ticks, seed=seed + k)
        i = np.arange(n, dtype=np.uint32) + base
        base += n
        assert mgr.init_batch(i, DT, 0.0, p0, type=te.MODEL_TYPES[name], Q=m["Q"], R=m["R"], P0=m["P"]) == n
        streams.append(meas)
        ids.append(i)
    bs = mgr.batches()
    assert [b.size for b in bs] == [n for _, n in parts]
    soa = [torch.stack([to_soa(meas[s], b) for s in range(ticks)]) for meas, b in zip(streams, bs)]
    return mgr, soa, ids


def _everything(mgr, ids):
    """per batch: state, covariance, time and measurement counter of every target (ids: one array per batch)"""
    torch.cuda.synchronize()
    out = []
    for i in ids:
        x, P = mgr.get_state_batch(i)
        out.append((x, P, np.array([mgr.getTime(int(k)) for k in i]), np.array([mgr.getNumberMeasurements(int(k)) for k in i])))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for b, (gb, wb) in enumerate(zip(got, want)):
        for g, w, what in zip(gb, wb, ("x", "P", "time", "measurements")):
            np.testing.assert_array_equal(g, w, err_msg="batch %d: %s" % (b, what))


def test_batch_cache_keeps_64_and_evicts_the_least_recently_used(models):
    """64 one-tick recordings over one measurement buffer, distinct by dt; a replay of the first makes it the most recently used,
    so the 65th recording takes the place of the second: the first replays without a new recording, the second records again."""
    parts = [("uniform_velocity", 3)]
    mgr, soa, ids = _manager(models, parts, 1, 21)
    twin, tsoa, _ = _manager(models, parts, 1, 21)
    b, tb = mgr.batches()[0], twin.batches()[0]
    dts = _dts(65)
    assert b.graph_recordings == 0
    calls = []

    def call(dt, want_recordings):
        b.step_sequence(dt, soa[0], use_graph=True)
        calls.append(dt)
        assert b.graph_recordings == want_recordings, (len(calls), b.graph_recordings, want_recordings)

    for k in range(64):
        call(dts[k], k + 1)
    call(dts[0], 64)    # a hit
    call(dts[64], 65)   # the cache is full: the least recently used recording (the second) goes
    call(dts[0], 65)    # the first was used last before that: it stayed
    call(dts[1], 66)    # the second did not
    for dt in calls:
        tb.step_sequence(dt, tsoa[0], use_graph=False)
    assert tb.graph_recordings == 0
    _same(_everything(mgr, ids), _everything(twin, ids))
    twin.close(); mgr.close()


@pytest.mark.parametrize("population", [True, False])
def test_manager_cache_evicts_and_records_again_with_the_same_bits(models, population):
    """Two-tick all-batches sequences over two non-empty batches, nine distinct time steps -- one more than the cache holds, so the
    first recording is evicted -- then the first again: states, clocks and measurement counters of every target equal those of
    a twin given the same calls eagerly.  population False: measured-pose rows keep the tick of all batches from being one launch,
    so the recordings are built with one branch per batch."""
    parts = [("uniform_velocity", 3), ("angular_rates", 3)]
    mgr, soa, ids = _manager(models, parts, 2, 31)
    twin, tsoa, _ = _manager(models, parts, 2, 31)
    if not population:
        mgr.set_keep_measurement(True)
        twin.set_keep_measurement(True)
    assert mgr.population_tick() is population and twin.population_tick() is population
    dts = _dts(9)
    for dt in dts + dts[:1]:
        mgr.step_sequence_all(dt, soa, use_graph=1)
        twin.step_sequence_all(dt, tsoa, use_graph=0)
    got, want = _everything(mgr, ids), _everything(twin, ids)
    for _, _, t, nm in want:
        assert (nm == 20).all() and len(set(t)) == 1 and t[0] > 0.0
    _same(got, want)
    twin.close(); mgr.close()
