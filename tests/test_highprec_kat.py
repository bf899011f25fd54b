"""The oracle, the NumPy twin and the HIP path against answers evaluated in 50-digit arithmetic from the reference's formulas
(tests/golden/make_highprec_kat.py -> tests/golden/highprec_kat.npz; four ticks per model: measured, measured, predict only,
measured, the measured yaw crossing +pi).  A restatement that MISREADS the reference is off in the leading digits; one that
only rounds differently is off by a few ulp amplified by the update's conditioning (1 - K with K ~ 0.999 in the first ticks
loses three digits).  Bounds, all fp64:
    x:  |dx| <= 1e-13 * max(1, |x|_inf)
    P:  |dP| <= 1e-13 * max|P|  and, entry by entry, |dP_ij| <= 2e-12 * |P_ij| + 1e-13 * sqrt(P_ii P_jj)
(the measured worst cases are printed by `pytest -s`).  The innovation nu = y - C x^- and NIS = nu^T S^-1 nu of the measured ticks
(oracle.OracleBatch.innovations) are held to the same fixture, with a bound that follows from the two above:
    nu:   |d nu_c| <= e = 1e-13 * max(1, |x|_inf)                      (y is exact; x^- is a state)
    NIS:  |d NIS| <= 2 |w|^T e + e^T |S^-1| e + 1e-13 max|P^-| (sum_c |w_c|)^2     w = S^-1 nu, S^-1, max|P^-| from the 50 digits
(first order in d nu and dS = dP^-[0:m,0:m], plus the quadratic remainder in d nu).  The same fixture holds 48 sphere intersections with the quartic's roots to
50 digits and the reference's selection rule (further down)."""
import os

import numpy as np
import pytest

import oracle
from conftest import synth_stream
from oracle import np_twin as tw

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ["uniform_velocity", "uniform_acceleration", "angular_rates", "angular_velocities"]


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "highprec_kat.npz"))


def x_err(x, xr):
    """|dx|_inf / max(1, |x|_inf) per target (x [N, n] or one vector), maximum over the batch (as `check` below)"""
    x, xr = np.asarray(x).reshape(-1, xr.shape[-1]), xr.reshape(-1, xr.shape[-1])
    return float((np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))).max())


def P_err(P, Pr):
    """|dP| / max|P| per target (P [N, n, n]), maximum over the batch"""
    P, Pr = np.asarray(P).reshape(-1, *Pr.shape[-2:]), Pr.reshape(-1, *Pr.shape[-2:])
    return float((np.abs(P - Pr).max(axis=(1, 2)) / np.abs(Pr).max(axis=(1, 2))).max())


def f32r(a):
    """the values an f32 holds, as doubles"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def check(tag, x, P, xk, Pk):
    ex = np.abs(x - xk).max() / max(1.0, np.abs(xk).max())
    eP = np.abs(P - Pk).max() / np.abs(Pk).max()
    d = np.sqrt(np.abs(np.diag(Pk)))
    bound = 2e-12 * np.abs(Pk) + 1e-13 * np.outer(d, d)
    worst = (np.abs(P - Pk) / np.maximum(bound, 1e-300)).max()
    print("%-44s x %.2e  P (norm) %.2e  P (entry / bound) %.3f" % (tag, ex, eP, worst))
    assert ex <= 1e-13, (tag, ex)
    assert eP <= 1e-13, (tag, eP)
    assert worst <= 1.0, (tag, worst)
    # structure: what the 50-digit evaluation leaves exactly zero stays exactly zero
    assert np.all(P[Pk == 0] == 0), tag


def drive(target, kat):
    dt = float(kat["dt"])
    for s, has in enumerate(kat["has"]):
        if has:
            target.add_measurement(dt, kat["meas"][s]) if hasattr(target, "add_measurement") else target.addMeasurement(dt, kat["meas"][s])
        else:
            target.update(dt)
        yield s


@pytest.mark.parametrize("name", MODELS)
def test_oracle_matches_the_high_precision_answers(models, kat, name):
    m = models[name]
    t = oracle.OracleTarget(m["model"], m["Q"], m["R"], m["P"], kat["p0"], float(kat["dt"]))
    for s in drive(t, kat):
        x, P = t.state()
        check("oracle %s tick %d" % (name, s + 1), x[0], P[0], kat["x_" + name][s], kat["P_" + name][s])


@pytest.mark.parametrize("name", MODELS)
def test_numpy_twin_matches_the_high_precision_answers(models, kat, name):
    m = models[name]
    t = tw.Target(m["model"], m["Q"], m["R"], m["P"], kat["p0"], float(kat["dt"]))
    dt = float(kat["dt"])
    for s, has in enumerate(kat["has"]):
        if has:
            t.add_measurement(dt, kat["meas"][s])
        else:
            t.update(dt)
        check("twin %s tick %d" % (name, s + 1), t.x, t.P, kat["x_" + name][s], kat["P_" + name][s])


def innov_check(tag, nu, nis, kat, key, s, x_scale, rel=1e-13, ulps=0):
    """nu [m], nis of tick s against the fixture's `key` rows (nu_<key> ...; module docstring).  rel: the bound on x and P the
    NIS bound is propagated from; ulps: double roundings granted on top (the f80 entry returns doubles, as the fixture holds)."""
    nk, sk, w, Sinv, pmax = (kat["gimbal_" + f if key == "gimbal" else f + "_" + key][s] for f in ("nu", "nis", "w", "Sinv", "pmax"))
    e = rel * max(1.0, x_scale)
    b_nu = e + ulps * np.spacing(np.abs(nk))
    b_nis = 2.0 * np.abs(w).sum() * e + e * e * np.abs(Sinv).sum() + rel * pmax * np.abs(w).sum() ** 2 + ulps * np.spacing(abs(sk))
    r_nu, r_nis = (np.abs(nu - nk) / b_nu).max(), abs(nis - sk) / b_nis
    print("%-44s NIS %.6g  |d nu| %.2e (%.3f of its bound)  |d NIS| %.2e (%.3f of its bound %.2e)"
          % (tag, sk, np.abs(nu - nk).max(), r_nu, abs(nis - sk), r_nis, b_nis))
    assert np.isfinite(nu).all() and np.isfinite(nis), tag
    assert r_nu <= 1.0, (tag, "nu", r_nu)
    assert r_nis <= 1.0, (tag, "NIS", r_nis)


@pytest.mark.parametrize("dtype", ["f64", "f80"])
@pytest.mark.parametrize("name", MODELS)
def test_oracle_innovations_match_the_high_precision_answers(models, kat, name, dtype):
    """OracleBatch.innovations before every step of the four-tick cases: fp64 within the bound of the module docstring; f80 within
    that bound at 1e-18 (what its x and P are held to below) plus one rounding to double of the value itself.  The
    predict-only tick gives the sentinels, asked with the mask."""
    m = models[name]
    dt = float(kat["dt"])
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], kat["p0"][None], dt, dtype=dtype)
    rel, ulps = (1e-13, 0) if dtype == "f64" else (1e-18, 1)
    for s, has in enumerate(kat["has"]):
        mask = np.array([1 if has else 0], dtype=np.uint8)
        nu, nis = orc.innovations(dt, kat["meas"][s][None], mask)
        if has:
            innov_check("%s oracle %s tick %d" % (dtype, name, s + 1), nu[0], nis[0], kat, name, s, np.abs(kat["x_" + name][s]).max(), rel, ulps)
        else:
            assert nis[0] == -1.0 and (nu[0] == 0.0).all()
            assert kat["nis_" + name][s] == -1.0
        orc.step(dt, kat["meas"][s][None], mask)


@pytest.mark.parametrize("dtype", ["f64", "f80"])
def test_oracle_innovations_through_the_gimbal_branches(models, kat, dtype):
    """The same through the gimbal branches of quatToRpy (angular rates; NIS of order 1e3: the measured attitude jumps)."""
    m = models["angular_rates"]
    dt = float(kat["dt"])
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], kat["p0"][None], dt, dtype=dtype)
    rel, ulps = (1e-13, 0) if dtype == "f64" else (1e-18, 1)
    for s in range(3):
        nu, nis = orc.innovations(dt, kat["gimbal_meas"][s][None])
        innov_check("%s oracle gimbal tick %d" % (dtype, s + 1), nu[0], nis[0], kat, "gimbal", s, np.abs(kat["gimbal_x"][s]).max(), rel, ulps)
        orc.step(dt, kat["gimbal_meas"][s][None])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_hip_path_matches_the_high_precision_answers(kat, name):
    """Through the reference's own C symbols (target_manager_new / _init / _update_meas / _update), fp64."""
    import target_estimation_amd as te
    from conftest import model_path
    mgr = te.TargetManager(model_path(name), dtype="f64")
    dt = float(kat["dt"])
    mgr.init(7, dt, 0.0, kat["p0"])
    for s, has in enumerate(kat["has"]):
        mgr.update(7, dt, kat["meas"][s] if has else None)
        x, P = mgr.get_state_batch([7])
        check("hip %s tick %d" % (name, s + 1), x[0], P[0], kat["x_" + name][s], kat["P_" + name][s])
    mgr.close()


# ---- sphere intersection: quartic roots to 50 digits, the reference's selection rule ---------------------------
def _ix_check(tag, kat, delta, pose):
    want_d, want_p = kat["ix_delta"], kat["ix_pose"]
    hit = want_d > -1
    assert ((delta > -1) == hit).all(), (tag, np.nonzero((delta > -1) != hit)[0])       # the same targets intersect (indices bit-exact)
    assert (delta[~hit] == -1).all()
    rel = np.abs(delta[hit] - want_d[hit]) / want_d[hit]
    dp = np.abs(pose[hit, :3] - want_p[hit, :3]).max()
    print("%-28s %d of %d intersect; max rel |d delta| %.2e, max |d position| %.2e" % (tag, hit.sum(), len(hit), rel.max(), dp))
    assert rel.max() <= 1e-12 and dp <= 1e-12, (tag, rel.max(), dp)
    np.testing.assert_array_equal(pose[:, 3:], np.tile([0, 0, 0, 1.0], (len(hit), 1)))     # uniform acceleration: identity orientation; misses: the initial pose


def test_oracle_intersections_match_the_high_precision_roots(models, kat):
    m = models["uniform_acceleration"]
    n = len(kat["ix_delta"])
    p0 = np.concatenate([kat["ix_p0"], np.tile([0, 0, 0, 1.0], (n, 1))], 1)
    v0 = np.concatenate([kat["ix_v0"], np.zeros((n, 3))], 1)
    a0 = np.concatenate([kat["ix_a0"], np.zeros((n, 3))], 1)
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, float(kat["dt"]), 0.0, v0, a0)
    ok, pose, delta = orc.intersection_pose(0.0, kat["ix_origin"], float(kat["ix_radius"]))
    assert (kat["ix_margin"] > 1e-3).all()            # the cases stay away from where a double-precision solver classifies by rounding
    assert 12 <= (kat["ix_delta"] > -1).sum() <= 40   # hits and misses both (zero acceleration, flying away, started inside)
    _ix_check("oracle", kat, delta, pose)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["one target at a time (the reference's call)", "batched"])
def test_hip_intersections_match_the_high_precision_roots(models, kat, path):
    import target_estimation_amd as te
    m = models["uniform_acceleration"]
    n = len(kat["ix_delta"])
    p0 = np.concatenate([kat["ix_p0"], np.tile([0, 0, 0, 1.0], (n, 1))], 1)
    v0 = np.concatenate([kat["ix_v0"], np.zeros((n, 3))], 1)
    a0 = np.concatenate([kat["ix_a0"], np.zeros((n, 3))], 1)
    mgr = te.TargetManager(dtype="f64")
    ids = np.arange(n, dtype=np.uint32) + 11
    assert mgr.init_batch(ids, float(kat["dt"]), 0.0, p0, v0, a0, type=m["model"], Q=m["Q"], R=m["R"], P0=m["P"]) == n
    origin, radius = kat["ix_origin"], float(kat["ix_radius"])
    if path == "batched":
        delta, pose, found = mgr.intersect_batch(ids, 0.0, origin, radius)
        assert found.all()
    else:
        delta, pose = np.empty(n), np.empty((n, 7))
        for i, id_ in enumerate(ids):
            ok, pose[i], delta[i] = mgr.intersection_pose(int(id_), 0.0, origin, radius)
            assert mgr.intersection_time(int(id_), 0.0, origin, radius) == delta[i]
    _ix_check("hip, " + path, kat, delta, pose)
    mgr.close()


# ---- derived outputs: updateTargetState's pose / twist / acceleration and the getters at t1 -----------------
def _out_check(tag, got, want, tol=2e-13):
    got = np.concatenate([np.asarray(g, dtype=float).ravel() for g in got])
    # a quaternion and its negative are the same rotation only to a caller; the reference's matrix -> quaternion branch fixes the sign,
    # and the fixture follows that branch: compare as is
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("%-52s max rel %.2e" % (tag, err.max()))
    assert err.max() <= tol, (tag, err.max(), int(err.argmax()))


@pytest.mark.parametrize("name", MODELS)
def test_oracle_outputs_match_the_high_precision_answers(models, kat, name):
    m = models[name]
    dt, ahead = float(kat["dt"]), float(kat["ahead"])
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], kat["p0"][None], dt)
    for s, has in enumerate(kat["has"]):
        orc.step(dt, kat["meas"][s][None], None if has else np.zeros(1, dtype=np.uint8))
        t1 = (s + 1) * dt + ahead
        want = kat["out_" + name][s]
        _out_check("oracle %s tick %d now" % (name, s + 1), (orc.pose(), orc.twist(), orc.acceleration()), want[:19])
        _out_check("oracle %s tick %d at t + %.4f" % (name, s + 1, ahead), (orc.pose_at(t1), orc.twist_at(t1)), want[19:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_hip_outputs_match_the_high_precision_answers(kat, name):
    """The reference's getters through the C symbols (own time) and the batched getter at t1 (extrapolation)."""
    import target_estimation_amd as te
    from conftest import model_path
    mgr = te.TargetManager(model_path(name), dtype="f64")
    dt, ahead = float(kat["dt"]), float(kat["ahead"])
    mgr.init(7, dt, 0.0, kat["p0"])
    for s, has in enumerate(kat["has"]):
        mgr.update(7, dt, kat["meas"][s] if has else None)
        want = kat["out_" + name][s]
        ok1, pose = mgr.getTargetPose(7)
        ok2, twist = mgr.getTargetTwist(7)
        ok3, acc = mgr.getTargetAcceleration(7)
        assert ok1 and ok2 and ok3
        _out_check("hip %s tick %d now" % (name, s + 1), (pose, twist, acc), want[:19])
        p1, t1w, _, found = mgr.get_est_batch([7], t1=(s + 1) * dt + ahead)
        assert found.all()
        _out_check("hip %s tick %d at t + %.4f" % (name, s + 1, ahead), (p1[0], t1w[0]), want[19:])
    mgr.close()


# ---- the gimbal branches of quatToRpy (geometry.hpp:156-169) -----------------------------------------------------------------------
def test_oracle_through_the_gimbal_branches(models, kat):
    """Measured pitch within 1e-3 of +pi/2, then of -pi/2 (|sin pitch| > 0.9999: roll = 0, yaw = 2 atan2(qz, qw)), then a regular
    attitude, through the angular-rates model: state, covariance and derived outputs against the 50-digit evaluation."""
    m = models["angular_rates"]
    dt, ahead = float(kat["dt"]), float(kat["ahead"])
    t = oracle.OracleTarget(m["model"], m["Q"], m["R"], m["P"], kat["p0"], dt)
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], kat["p0"][None], dt)
    for s in range(3):
        t.add_measurement(dt, kat["gimbal_meas"][s])
        orc.step(dt, kat["gimbal_meas"][s][None])
        x, P = t.state()
        check("oracle gimbal tick %d" % (s + 1), x[0], P[0], kat["gimbal_x"][s], kat["gimbal_P"][s])
        want = kat["gimbal_out"][s]
        _out_check("oracle gimbal tick %d now" % (s + 1), (orc.pose(), orc.twist(), orc.acceleration()), want[:19])
        _out_check("oracle gimbal tick %d ahead" % (s + 1), (orc.pose_at((s + 1) * dt + ahead), orc.twist_at((s + 1) * dt + ahead)), want[19:])


@pytest.mark.gpu
def test_hip_through_the_gimbal_branches(kat):
    import target_estimation_amd as te
    from conftest import model_path
    mgr = te.TargetManager(model_path("angular_rates"), dtype="f64")
    dt, ahead = float(kat["dt"]), float(kat["ahead"])
    mgr.init(3, dt, 0.0, kat["p0"])
    for s in range(3):
        mgr.update(3, dt, kat["gimbal_meas"][s])
        x, P = mgr.get_state_batch([3])
        check("hip gimbal tick %d" % (s + 1), x[0], P[0], kat["gimbal_x"][s], kat["gimbal_P"][s])
        want = kat["gimbal_out"][s]
        _out_check("hip gimbal tick %d now" % (s + 1), (mgr.getTargetPose(3)[1], mgr.getTargetTwist(3)[1], mgr.getTargetAcceleration(3)[1]), want[:19])
        p1, t1w, _, _ = mgr.get_est_batch([3], t1=(s + 1) * dt + ahead)
        _out_check("hip gimbal tick %d ahead" % (s + 1), (p1[0], t1w[0]), want[19:])
    mgr.close()


# ---- the extended-precision (f80, long double) oracle: the yardstick of tests/test_gpu_precision.py --------------------------------
def test_long_double_has_a_64_bit_mantissa():
    """The f80 instantiation is only a yardstick if long double is wider than double (x87 extended: 64 bits)."""
    dig = oracle.load().orc_long_double_mant_dig()
    assert dig >= 64, ("long double has a %d-bit mantissa on this platform: the f80 oracle would be no more precise than the "
                       "f64 one, and tests/test_gpu_precision.py would measure nothing" % dig)


@pytest.mark.parametrize("name", MODELS)
def test_f80_oracle_matches_the_high_precision_answers(models, kat, name):
    """Measured: 0 to 1.3e-21 (x and P, relative)."""
    m = models[name]
    t = oracle.OracleTarget(m["model"], m["Q"], m["R"], m["P"], kat["p0"], float(kat["dt"]), dtype="f80")
    for s in drive(t, kat):
        x, P = t.state()
        xk, Pk = kat["x_" + name][s], kat["P_" + name][s]
        ex, eP = x_err(x[0], xk), P_err(P[0], Pk)
        print("f80 oracle %-22s tick %d  x %.2e  P %.2e" % (name, s + 1, ex, eP))
        assert ex <= 1e-18 and eP <= 1e-18, (name, s + 1, ex, eP)
        assert np.all(P[0][Pk == 0] == 0), name


def test_f80_oracle_intersections_match_the_high_precision_roots(models, kat):
    m = models["uniform_acceleration"]
    n = len(kat["ix_delta"])
    p0 = np.concatenate([kat["ix_p0"], np.tile([0, 0, 0, 1.0], (n, 1))], 1)
    v0 = np.concatenate([kat["ix_v0"], np.zeros((n, 3))], 1)
    a0 = np.concatenate([kat["ix_a0"], np.zeros((n, 3))], 1)
    orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, float(kat["dt"]), 0.0, v0, a0, dtype="f80")
    ok, pose, delta = orc.intersection_pose(0.0, kat["ix_origin"], float(kat["ix_radius"]))
    _ix_check("f80 oracle", kat, delta, pose)


# What a faithful implementation errs by against the f80 oracle on synth_stream (200 targets), measured: f64 at tick 100,
# f32 (f32-rounded inputs on both sides) at tick 300.  x: |dx| / max(1, |x|); P: |dP| / max|P|; per target, batch maxima.
FAITHFUL = {"uniform_velocity": dict(f64=(6e-14, 1e-15), f32=(2e-5, 3e-6)),
            "uniform_acceleration": dict(f64=(7e-14, 8e-15), f32=(1.7e-4, 7e-6)),
            "angular_rates": dict(f64=(1.7e-13, 5e-15), f32=(1.7e-4, 4e-6)),
            "angular_velocities": dict(f64=(6e-14, 5e-15), f32=(2e-5, 1e-5))}


@pytest.mark.parametrize("name", MODELS)
def test_f64_and_f32_oracles_stay_near_the_f80_oracle(models, name):
    """Pins the 'faithful error' the GPU precision matrix holds every kernel to a small multiple of: over 300 ticks the f64
    and f32 oracles stay within 4x the figures above (f64 at tick 100, f32 at tick 300) of the f80 oracle, and not absurdly far inside them either (a yardstick
    that agreed with f64 to the last bit would be no yardstick)."""
    m = models[name]
    N, steps, dt = 200, 300, 0.004
    p0, meas = synth_stream(name, N, steps, seed=23)
    p032, meas32 = f32r(p0), f32r(meas)
    mk = lambda d, p: oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p, dt, dtype=d)  # noqa: E731
    o64, o80, o32, o80r = mk("f64", p0), mk("f80", p0), mk("f32", p032), mk("f80", p032)
    for s in range(steps):
        for o, mm in ((o64, meas), (o80, meas), (o32, meas32), (o80r, meas32)):
            o.step(dt, mm[s], nthreads=8)
        if s + 1 in (100, steps):
            (x64, P64), (x80, P80) = o64.state(), o80.state()
            (x32, P32), (x80r, P80r) = o32.state(), o80r.state()
            e64, e32 = (x_err(x64, x80), P_err(P64, P80)), (x_err(x32, x80r), P_err(P32, P80r))
            print("faithful %-22s tick %3d  f64 x %.2e P %.2e   f32 x %.2e P %.2e" % (name, s + 1, *e64, *e32))
            if s + 1 == 100:
                fx, fP = FAITHFUL[name]["f64"]
                assert e64[0] <= 4 * fx and e64[1] <= 4 * fP, (name, s + 1, e64)
                assert e64[0] >= 1e-17 and e64[1] >= 1e-18, (name, s + 1, e64)
    fx, fP = FAITHFUL[name]["f32"]
    assert e32[0] <= 4 * fx and e32[1] <= 4 * fP, (name, e32)
    assert e32[0] >= 1e-9 and e32[1] >= 1e-10, (name, e32)
