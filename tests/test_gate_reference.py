"""The conditions the GPU tests of the NIS validation gate rest on (tests/test_gpu_gate.py), checked on the gated twin of
tests/gate_ref.py alone -- no library, no GPU.  It guards the inputs, not the feature.

gamma = 300: every +0.5 m outlier pair and every yaw-spike pair is rejected, no clean pair is, and every measured pair's NIS lies
at least 10 times its innov_stream_ref bound from gamma in fp32 and in fp64 -- so a device NIS inside its bound decides as the
twin does, and the GPU comparison at gamma = 300 excludes no pair.
gamma = the chi-square 0.99 quantile: the stream's 1 cm noise against the shipped R rejects a real share of the measurements
(between 5 % and 60 % of the measured pairs), so "gated equals masked" there exercises both branches in every wavefront."""
import numpy as np
import pytest

import gate_ref
from conftest import HARNESS_ORDER


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_gamma_300_separates_the_outliers_with_a_margin(name):
    p0, meas, mask, outlier, spikes = gate_ref.stream(name)
    want = gate_ref.reference(name, gate_ref.GAMMA_FAR)
    has = mask.astype(bool)
    spike = np.zeros_like(has)
    for s, j in spikes:
        spike[s, j] = True
    assert (spike & outlier).sum() == 0 and (spike <= has).all() and (outlier <= has).all()
    assert len(spikes) == (4 if gate_ref.m_of(name) == 6 else 0)
    bad = outlier | spike
    rejected = has & ~want["acc"]
    print("%s: outlier pairs rejected %d of %d, spike pairs %d of %d, clean measured pairs rejected %d of %d" %
          (name, (rejected & outlier).sum(), outlier.sum(), (rejected & spike).sum(), spike.sum(), (rejected & ~bad).sum(), (has & ~bad).sum()))
    assert outlier.sum() > 100
    assert (rejected & bad).sum() == bad.sum(), "an outlier pair passes the gate"
    assert (rejected & ~bad).sum() == 0, "a clean pair is rejected"
    for dtype in ("f32", "f64"):
        r = gate_ref.margin(want, mask, dtype, gate_ref.GAMMA_FAR)
        print("%s %s: smallest |NIS - gamma| / bound %.3g (spike pairs %s)" % (name, dtype, r.min(), [float("%.3g" % r[s, j]) for s, j in spikes]))
        assert r.min() >= 10.0, "a pair's NIS is within 10 bounds of gamma"
    # the clean measurements behind the spikes are accepted: the unwrap memory did not advance on a rejection
    for s, j in spikes:
        assert want["acc"][gate_ref.SPIKE_TICKS[-1] + 1, j] and want["acc"][gate_ref.SPIKE_TICKS[-1] + 2, j]
    assert np.isfinite(want["x"]).all() and np.isfinite(want["P"]).all()


@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_chi_square_gate_rejects_a_real_share(name):
    p0, meas, mask, outlier, spikes = gate_ref.stream(name)
    want = gate_ref.reference(name, gate_ref.CHI2_99[gate_ref.m_of(name)])
    has = mask.astype(bool)
    share = (has & ~want["acc"]).sum() / has.sum()
    print("%s: rejected share of measured pairs at the 0.99 quantile %.1f %%" % (name, 100 * share))
    assert 0.05 <= share <= 0.60
