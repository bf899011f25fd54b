"""CPU only: the conditions the GPU tests of the re-acquisition (tests/test_gpu_reacquire.py) rest on, asserted on the twin of
tests/reacquire_ref.py for all four models: the gate alone locks the jumped targets out; K = 3 brings every one of them back;
at gamma = 300 every measured pair is at least 10 bounds from the gate, so the numeric GPU test leaves no pair out; and the
chi-square 0.99 gate gives the bit-exact test real work."""
import numpy as np
import pytest

import gate_ref
import innov_stream_ref as ref
import reacquire_ref as rq
from conftest import HARNESS_ORDER


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_far_gate_with_k3_reacquires_every_jumped_target(name):
    want = rq.reference(name, gate_ref.GAMMA_FAR, 3)
    init = (want["event"] & 0x80) != 0
    print("%s: %d re-initialisations, %d on the jumped targets" % (name, init.sum(), init[:, rq.JUMPED].sum()))
    assert init.sum() == 26
    assert init[:, rq.JUMPED].sum() == 24
    assert init[:, rq.JUMPED].any(0).all(), "a jumped target is never re-initialised"
    assert ((want["event"][init] & 0x7F) == 3).all()
    assert not init[:rq.JUMP_TICK + 2, rq.JUMPED].any()


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_without_reacquisition_the_jumped_targets_are_locked_out(name):
    want = rq.reference(name, gate_ref.GAMMA_FAR, 0)
    _, _, mask, _, _ = rq.stream(name)
    has = mask.astype(bool)[rq.JUMP_TICK:, rq.JUMPED]
    assert has.sum() > 100
    assert not want["acc"][rq.JUMP_TICK:, rq.JUMPED][has].any(), "a jumped target's measurement is accepted after the jump"
    assert not (want["event"] & 0x80).any()
    runs = want["run"][rq.JUMPED]
    # the lock-out length: every measured tick since the jump (more where an outlier was rejected just ahead of it)
    assert (runs >= has.sum(0)).all() and (runs <= has.sum(0) + 2).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_every_pair_is_far_from_the_far_gate(name, dtype):
    gamma = gate_ref.GAMMA_FAR
    want = rq.reference(name, gamma, 3)
    _, _, mask, _, _ = rq.stream(name)
    r = gate_ref.margin(want, mask, dtype, gamma)
    has = mask.astype(bool)
    rel = (np.abs(want["nis"] - gamma) / gamma)[has].min()
    print("%s %s: least |NIS - gamma| = %.3g bounds, %.3g gamma" % (name, dtype, r.min(), rel))
    assert r.min() >= 10.0
    assert rel >= 0.5


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_the_chi_square_gate_reinitialises_often(name):
    want = rq.reference(name, gate_ref.CHI2_99[gate_ref.m_of(name)], 3)
    k = int(((want["event"] & 0x80) != 0).sum())
    print("%s: %d re-initialisations at the chi-square 0.99 gate" % (name, k))
    assert k >= 50
