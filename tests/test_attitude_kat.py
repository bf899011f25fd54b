"""The CPU oracle (f32 / f64 / f80) and the NumPy twin against the 50-digit attitude fixture (tests/golden/make_attitude_kat.py ->
tests/golden/attitude_kat.npz): pose7 / twist6 / acceleration6 at the target's own time, at four offsets and after one to three
predict-only ticks, over all four branches of the matrix -> quaternion rule, per group (tests/attitude_kat_ref.py).

Ceiling of a group = 4 x the error measured on the machine the fixture was made on (profiles/attitude_kat_tolerances.txt, the
`cpu` lines; `python tests/attitude_kat_ref.py` rewrites them); the factor covers libm differences between machines.  STRICT rows
are compared as they are, the quaternion's sign included; the rest as rotations.  `pytest -s` prints every group's error."""
import os
import sys

import numpy as np
import pytest

import oracle
import attitude_kat_ref as ak

L = np.longdouble


def _ld_decisions(rpy):
    """trace, diagonal and cos(pitch) of quat_to_rot(rpy_to_quat(rpy)) in long double, [n] each"""
    h = rpy.astype(L) / 2
    c, s = np.cos(h), np.sin(h)
    w = c[:, 0] * c[:, 1] * c[:, 2] + s[:, 0] * s[:, 1] * s[:, 2]
    x = s[:, 0] * c[:, 1] * c[:, 2] - c[:, 0] * s[:, 1] * s[:, 2]
    y = c[:, 0] * s[:, 1] * c[:, 2] + s[:, 0] * c[:, 1] * s[:, 2]
    z = c[:, 0] * c[:, 1] * s[:, 2] - s[:, 0] * s[:, 1] * c[:, 2]
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    diag = np.stack([1 - 2 * (y * y + z * z), 1 - 2 * (x * x + z * z), 1 - 2 * (x * x + y * y)], 1)
    trace = diag.sum(1)
    i = np.where(diag[:, 1] > diag[:, 0], 1, 0)
    i = np.where(diag[:, 2] > diag[np.arange(len(i)), i], 2, i)
    return trace, np.where(trace > 0, 0, 1 + i), np.cos(rpy[:, 1].astype(L))


def _ld_init_rpy(p0):
    """the init conversion (normalise, quat_to_rpy with its gimbal branches) in long double: rpy [n,3], |sin pitch| - 0.9999"""
    q = p0[:, 3:7].astype(L)
    q = q / np.sqrt((q * q).sum(1))[:, None]
    x, y, z, w = q.T
    sp = -2 * (x * z - w * y)
    pi = L(float(np.pi))          # the reference's M_PI
    reg = np.stack([np.arctan2(2 * (y * z + w * x), w * w - x * x - y * y + z * z), np.arcsin(np.clip(sp, -1, 1)),
                    np.arctan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z)], 1)
    gim = np.stack([np.zeros_like(sp), np.sign(sp) * pi / 2, 2 * np.arctan2(z, w)], 1)
    return np.where((np.abs(sp) > L("0.9999"))[:, None], gim, reg), np.abs(sp) - L("0.9999")


def _same_sign(a, b):
    return bool(np.all((np.asarray(a, dtype=np.float64) > 0) == (np.asarray(b, dtype=np.float64) > 0)))


@pytest.mark.parametrize("name", ak.ANGULAR)
def test_the_fixture_meets_its_own_conditions(name):
    """Sizes, the branch counts, the strict share, >= 24 strict rows in every group, f32-exact inputs, and every stored decision
    value of a strict row recomputed in long double with the same sign (the branch with the same outcome)."""
    m = ak.Model(name)
    assert m.n % 64 and m.n % 10 and 400 <= m.n <= 500
    M = len(m.tick_cases)
    assert M % 64 and M % 10 and M > 64
    for a in (m.p0, m.v0, m.a0, np.array([m.dt]), m.offsets):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    norm = np.linalg.norm(m.p0[:, 3:7], axis=1)
    assert norm.min() < 0.7 and norm.max() > 1.5 and (m.p0[:, 6] < 0).sum() > 100 and (m.p0[:, 6] > 0).sum() > 100
    assert set(m.offsets.tolist()) == {0.0, 0.0625, -0.03125, 2.5}
    counts = np.bincount(m.branch_now[~m.gimbal], minlength=4)
    print("%s branches (trace, i = 0, 1, 2) now: %s, over the tick rows: %s" % (name, counts, np.bincount(m.branch_k.ravel(), minlength=4)))
    assert (counts >= 64).all(), counts
    rows = np.concatenate([m.strict_now, m.strict_now[~m.gimbal], m.strict_k.ravel()])
    assert rows.mean() >= 0.90, rows.mean()
    for g in range(12):
        strict = (m.strict_now[m.group_now == g], m.strict_now[m.group_at == g], m.strict_k[m.group_k == g])[g // 4]
        assert strict.sum() >= 24, (m.group_names[g], int(strict.sum()))
    assert m.gimbal.sum() >= 24 and not m.strict_now[m.gimbal].any()
    if name == "angular_velocities":
        w = np.linalg.norm(m.v0[:, 3:], axis=1)
        assert (w == 0).sum() >= 24 and (w == 2.0 ** -40).sum() >= 24 and w.max() > 2.5
        assert (np.linalg.norm(m.v0[m.tick_cases, 3:], axis=1) == 2.0 ** -40).sum() >= 8
    else:
        past = (np.abs(m.x_k[:, :, 4]) > np.pi / 2).any(axis=0)
        assert past.sum() >= 24 and np.abs(m.v0[:, 4]).max() > 2.9      # state pitch past +-pi/2: only predict ticks get there
    # the stored decisions against a long double evaluation from the inputs (now) and from the stored states (ticks)
    d = m.d_now
    strict_by_d = (np.abs(d[:, 0]) >= 1e-5) & (d[:, 1] >= 1e-5) & (np.abs(d[:, 2]) >= 1e-5) & (d[:, 3] >= 1e-5) & (d[:, 4] >= 1e-5) & (np.abs(d[:, 5]) >= 0.05)
    assert np.array_equal(strict_by_d, m.strict_now)
    rpy, thr = _ld_init_rpy(m.p0)
    assert _same_sign(thr, d[:, 0]) and np.array_equal(thr > 0, m.gimbal)        # (nobody is within 1e-5 of the threshold)
    assert (np.abs(d[:, 0]) >= 1e-5).all()
    trace, branch, cosp = _ld_decisions(rpy)
    s = m.strict_now
    assert _same_sign(trace[s], d[s, 2]) and _same_sign(cosp[s], d[s, 5]) and np.array_equal(branch[s], m.branch_now[s])
    for k in range(3):
        trace, branch, cosp = _ld_decisions(m.x_k[k, :, 3:6])
        s, dk = m.strict_k[k], m.d_k[k]
        assert _same_sign(trace[s], dk[s, 0]) and np.array_equal(branch[s], m.branch_k[k][s])
        if name == "angular_rates":      # (the EKF rows store the least |cos| along the way)
            assert _same_sign(cosp[s], dk[s, 3])
        assert (np.abs(cosp[s].astype(np.float64)) >= 0.05 - 1e-6).all()
        d0 = m.d_now[m.tick_cases]
        by_d = (np.abs(d0[:, 0]) >= 1e-5) & (d0[:, 1] >= 1e-5) & (np.abs(dk[:, 0]) >= 1e-5) & (dk[:, 1] >= 1e-5) & (dk[:, 2] >= 1e-5) & (np.abs(dk[:, 3]) >= 0.05)
        assert np.array_equal(by_d, s)


def test_the_generator_reproduces_the_committed_fixture():
    """One model's arrays regenerated (mpmath, 50 digits) equal the committed ones bit for bit."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(ak.HERE, "golden"))
    import make_attitude_kat as gen
    fresh = gen.model_rows("angular_velocities")
    with np.load(os.path.join(ak.HERE, "golden", "attitude_kat.npz")) as z:
        for k, v in fresh.items():
            assert z[k].dtype == np.asarray(v).dtype and np.array_equal(z[k], v), k
    assert os.path.getsize(os.path.join(ak.HERE, "golden", "attitude_kat.npz")) <= os.path.getsize(os.path.join(ak.HERE, "golden", "quartic_cases.npz"))


def _hold(name, prec, errs):
    ceil = ak.read_ceilings()
    want = {g for (n, p, g) in ceil if n == name and p == prec}
    assert set(errs) == want, (name, prec, sorted(set(errs) ^ want))
    bad = []
    for g in sorted(errs):
        measured, c = ceil[(name, prec, g)]
        assert c == pytest.approx(ak.ceiling(measured), rel=1e-3), (name, prec, g)       # the file's ceiling is the rule's
        print("[attitude] %-20s %-4s %-14s error %.3e  ceiling %.3e" % (name, prec, g, errs[g], c))
        if not errs[g] <= c:
            bad.append((g, errs[g], c))
    assert not bad, (name, prec, bad)


@pytest.mark.parametrize("prec", ["f32", "f64", "f80"])
@pytest.mark.parametrize("name", ak.ANGULAR + ak.CONTROLS)
def test_oracle_matches_the_attitude_answers(models, name, prec):
    _hold(name, prec, ak.oracle_errors(oracle, models, name, prec))


@pytest.mark.parametrize("name", ak.ANGULAR + ak.CONTROLS)
def test_numpy_twin_matches_the_attitude_answers(models, name):
    _hold(name, "twin", ak.twin_errors(models, name))


@pytest.mark.parametrize("name", ak.ANGULAR + ak.CONTROLS)
def test_f80_is_not_worse_than_f64_in_any_group(models, name):
    """The yardstick of the GPU tests' "faithful" error: in no group is the f80 oracle further from the 50 digits than the f64
    one (both hand over doubles: one rounding, 2^-53, is granted where f64 happens to land on the fixture's double)."""
    e64, e80 = ak.oracle_errors(oracle, models, name, "f64"), ak.oracle_errors(oracle, models, name, "f80")
    for g in e64:
        assert e80[g] <= e64[g] + ak.ROUNDING, (name, g, e80[g], e64[g])
