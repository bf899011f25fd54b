"""CPU-only: the stream that tests/test_gpu_update_gate.py steps by id under the policy (300, K = 3) exercises every case of the
rule -- re-initialisations, rejections without one, targets whose run is not zero at the end -- for all four models, so the GPU
tests cannot pass vacuously; and the by-id rule used there is reacquire_ref.event_rule."""
import numpy as np
import pytest

import reacquire_ref as rq
from conftest import HARNESS_ORDER

# computed on the CPU twin: (re-initialisations, rejections without re-initialisation, targets with a non-zero final run)
WANT = {"uniform_velocity": (26, 248, 15), "uniform_acceleration": (26, 248, 15), "angular_rates": (26, 252, 15), "angular_velocities": (26, 252, 15)}


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_the_stream_exercises_every_case(name):
    want = rq.reference(name, 300.0, 3)
    ev, run = want["event"], want["run"]
    init = (ev & 0x80) != 0
    got = (int(init.sum()), int(((ev != 0) & ~init).sum()), int((run != 0).sum()))
    print(name, got)
    assert got[0] >= 1 and got[1] >= 1 and got[2] >= 1
    assert got == WANT[name]
    _, _, mask, _, _ = rq.stream(name)
    measured_later = [(s, j) for s, j in zip(*np.nonzero(init)) if mask[s + 1:, j].any()]
    assert measured_later, "no re-initialised target is measured again"
    assert (ev[~mask.astype(bool)] == 0).all()
    assert want["acc"].sum() >= 1000


def test_event_rule_table():
    assert rq.event_rule(5, False, False, True, 3) == (5, 0, False)
    assert rq.event_rule(5, True, True, True, 3) == (0, 0, False)
    assert rq.event_rule(1, True, False, True, 3) == (2, 2, False)
    assert rq.event_rule(2, True, False, True, 3) == (0, 0x83, True)
    assert rq.event_rule(2, True, False, False, 3) == (3, 3, False)
    assert rq.event_rule(127, True, False, True, 0) == (127, 127, False)
