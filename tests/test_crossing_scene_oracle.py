"""CPU-only: the oracle alone on the scene of the crossing-covariance tests (tests/crossing_scene.py).  The GPU tests compare the
device's rows with the oracle's on this scene and rely on what is asserted here: who crosses the sphere and who does not is the
scene's decision (every target aimed to miss has intersection_time == -1, every other one crosses, none is left out), every
crossing is far from tangential (|n . v_c| >= 0.1, so sigma_t is a division by a well-determined number) and every crosser's
radial variance n^T Sigma n is positive."""
import numpy as np
import pytest

import oracle
import crossing_scene as cs

SIZES = [1, 63, 64, 65, 130]


def test_the_mask_keeps_whole_tiles_and_splits_others():
    has = cs.has_mask(130)
    per_tile = [has[:, t * 64:(t + 1) * 64] for t in range(3)]
    assert per_tile[0].all() and per_tile[2].all()                   # tiles 0 and 2 (the partial one): measured on every tick
    assert not per_tile[1].all() and per_tile[1].any(axis=1).all()   # tile 1 is split on some ticks, never empty
    assert cs.has_mask(64).all()
    miss = cs.aimed_to_miss(130)
    assert miss.sum() == 26 and miss[2] and not miss[0]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", cs.CROSSING_MODELS)
def test_scene_conditions(models, name, dtype):
    for n in SIZES:
        scene = cs.build(n)
        orc = cs.oracle_batch(oracle, models[name], scene, dtype)
        times = orc.times()
        assert np.all(times == times[0])
        delta = orc.intersection_time(times[0], cs.ORIGIN, cs.RADIUS)
        miss = scene["miss"]
        assert np.all(delta[miss] == -1.0), (name, n, delta[miss])
        assert np.all(delta[~miss] >= 0.0), (name, n, delta[~miss].min())
        assert np.all(delta[~miss] < 2.0)
        if (~miss).sum() == 0:
            continue
        rows = cs.oracle_rows(orc, delta)
        sr, st, nv, dist, form = cs.sigma_reference(rows["Sigma"][~miss], rows["pc"][~miss], rows["vc"][~miss])
        assert np.all(nv >= 0.1), (name, n, nv.min())
        assert np.all(form > 0), (name, n, form.min())
        assert np.all(np.abs(dist - cs.RADIUS) < 1e-3), (name, n, np.abs(dist - cs.RADIUS).max())   # p_c is on the sphere
        assert np.all(np.isfinite(np.asarray(sr, float))) and np.all(np.isfinite(np.asarray(st, float)))
        # the separable models keep exact zeros between the axes
        off = rows["Sigma"][~miss][:, [0, 0, 1], [1, 2, 2]]
        assert np.all(off == 0.0)
