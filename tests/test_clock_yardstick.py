"""The yardstick of tests/test_gpu_clock.py on the CPU: the oracle's clock is the reference's sequential double sum
t_ = t_ + dt (target_interface.cpp:151) bit for bit, and the exact time it is measured against is what it claims."""
import math
from fractions import Fraction

import numpy as np

import oracle


def _orc(t0, dtype="f64"):
    m = oracle.MODELS["uniform_velocity"]
    n, _ = oracle.MODEL_DIMS[m]
    return oracle.OracleBatch(m, np.eye(n) * 1e-3, np.eye(3) * 1e-2, np.eye(n), np.array([[1.0, 2.0, 3.0, 0, 0, 0, 1]]), 0.004, t0,
                              dtype=dtype)


def test_oracle_clock_is_the_sequential_sum_at_250_hz():
    dt, ticks = 0.004, 100000
    for t0 in (0.0, 86400.123, 1.7e9):
        orc = _orc(t0)
        seq = np.cumsum(np.concatenate([[t0], np.full(ticks, dt)]))   # np.cumsum adds left to right: the same roundings
        ref = t0
        for s in range(ticks):
            orc.step(dt, None if s % 3 else np.array([[1.0, 2.0, 3.0, 0, 0, 0, 1]]))   # predict-only and measured updates
            ref += dt
            if s % 9973 == 0 or s == ticks - 1:
                assert orc.times()[0] == ref == seq[s + 1], (t0, s)
        assert orc.times()[0] == seq[-1]
        exact = Fraction(t0) + ticks * Fraction(dt)
        err = abs(Fraction(seq[-1]) - exact)
        assert err > 0 or t0 == 0.0          # at 250 Hz the sequential sum does drift from exact time ...
        assert err < ticks * math.ulp(seq[-1])   # ... by at most half an ulp per update


def test_oracle_clock_in_every_precision_and_the_time_setter():
    for d in ("f64", "f32", "f80"):
        orc = _orc(5.0, d)
        for _ in range(10):
            orc.step(1.0 / 60.0)
        want = 5.0
        for _ in range(10):
            want += 1.0 / 60.0
        assert orc.times()[0] == want, d      # the time is a double whatever the filter precision
        p = orc.pose_at(want + 0.25)
        orc.set_times(0.0)
        np.testing.assert_array_equal(orc.pose_at(0.25), p)   # the getters at t1 see t1 - t_ only
        assert orc.times()[0] == 0.0


def test_exact_time_of_a_dyadic_step_is_the_double_sum():
    """2^-8 (the precision matrix's step) is the control: every partial sum is exact, so t_ref == t_exact."""
    t, exact = 86400.0, Fraction(86400)
    for _ in range(10000):
        t += 2.0 ** -8
        exact += Fraction(2) ** -8
    assert Fraction(t) == exact
