"""CPU-only: the schedule and the twin behind tests/test_gpu_dt_schedule.py (tests/dt_schedule_ref.py).  The gated GPU tests are
vacuous unless the gate, with the twin stepped at dt[s], rejects and re-initialises: at least 10 rejections and 3
re-initialisations per model (the counts are in that module's docstring)."""
import numpy as np
import pytest

import dt_schedule_ref as ds
import gate_ref
import reacquire_ref as rq
from conftest import HARNESS_ORDER


def test_the_schedule():
    s = ds.SCHEDULE
    assert s.shape == (rq.TICKS,) and not s.flags.writeable
    assert s[ds.ZERO_TICK] == 0.0 and s[ds.LONG_TICK] == 3.0 * rq.DT
    rest = np.delete(s, [ds.ZERO_TICK, ds.LONG_TICK]) / rq.DT
    assert (rest >= 0.25).all() and (rest <= 2.0).all() and len(set(rest)) == len(rest)
    np.testing.assert_array_equal(ds.make_schedule(), s)


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_the_gated_run_is_not_vacuous(name):
    gamma = gate_ref.CHI2_99[gate_ref.m_of(name)]
    t = ds.twin(name, gamma, 3)
    mask = rq.stream(name)[2].astype(bool)
    rejected, reinit = int((mask & ~t["acc"]).sum()), int(((t["event"] & 0x80) != 0).sum())
    print("%s: %d rejections, %d re-initialisations of %d measurements" % (name, rejected, reinit, mask.sum()))
    assert rejected >= 10 and reinit >= 3
    # the decisions differ from those of the fixed-dt stream
    assert not np.array_equal(t["event"], rq.reference(name, gamma, 3)["event"])


def test_an_all_equal_schedule_is_the_fixed_dt_twin(models):
    name = "uniform_velocity"
    mdl = models[name]
    p0, meas, mask, _, _ = rq.stream(name)
    got = ds.twin_schedule(mdl["model"], mdl["Q"], mdl["R"], mdl["P"], p0, meas, mask, np.full(rq.TICKS, rq.DT), 300.0, 3)
    want = rq.reference(name, 300.0, 3)
    for k in ("x", "P", "nis", "nu", "event", "run", "acc"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
