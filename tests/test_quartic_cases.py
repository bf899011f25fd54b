"""Hard sphere scenes with 50-digit answers (tests/golden/make_quartic_cases.py -> tests/golden/quartic_cases.npz), the acceptance
rule every solver of the intersection quartic is held to on them, and the CPU sides of it: the fixture's own conditions, the
f64 / f32 oracle (long-double Aberth roots) and te_quartic.hpp compiled for the host.  tests/test_gpu_quartic_cases.py holds the
device code to the same rule through every kernel that inlines the solver.

The reference of a case is the quartic with the DOUBLE coefficients the kernels form (kf_aux.hpp sphere_query_values, left to
right, no fusing), its roots to 50 digits, and the reference's selection rule (|imag| < 1e-10 is real; the smallest real part;
none or negative -> -1; a zero leading coefficient -> -1).  m is the LOCAL margin of a case: the smallest |Im z| / |z| over its
non-real roots and gap / max(|r_j|, |r_j+1|) over neighbouring real roots.  TAU = 2^-20 separates clear cases from unclear ones:
a one-ulp change of a coefficient splits a double root by about sqrt(2^-53) |z| = 1e-8 |z|; TAU is 90 times that.

The rule (accept below), eps = 2^-52, eps_T the epsilon of the state's precision:
  clear case (m > TAU)   hit / miss as the reference, no exceptions; a miss is exactly -1 with the identity pose; c0 == 0 gives
                         exactly 0.0 or -1;  |d - want| <= K err_oracle + 8 eps |want| / min(1, m)  with err_oracle the error of
                         the project's own oracle in the family (its largest absolute error, or its largest error in units of
                         the second term, whichever gives less) and K = 8 as in tests/test_gpu_precision.py;  position within
                         (K err_oracle + 8 eps_T |want| / min(1, m)) (|v| + |a| want) + 8 eps_T max(1, |p|)
  unclear case           -1 unless the leftmost real root is clear and non-negative; d >= 0 within TAU max(|d|, tiny) of the real
                         part of a root with |Im z| <= TAU |z|, |p(d)| <= 64 2^-53 sum |c_k| d^k in long double, no clear real root
                         to its left
  no NaN anywhere.
`pytest -s` prints every family's worst error in units of 8 eps |want| / min(1, m), for the solver under test and the oracle.
Measured (profiles/quartic_cases_ratios.txt): the host build and the MI355X kernels reach 0.122 of that unit at the most (one
ulp of the crossing time), f64 and f32 state alike; the oracle 0.019.  K multiplies the oracle's figure, never the solver's.

The fixture is 270 KB, under the limit for a committed file: a case stores about 95 bytes that do not compress (nine inputs, and
twice a time, a position and a margin)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "quartic_cases.npz")
TAU = 2.0 ** -20
K = 8.0
EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}
TINY = float(np.finfo(np.float64).tiny)
# families whose cases are unclear by construction / all misses by construction (see test_fixture_conditions)
UNCLEAR_FAMILY = "tangent"

_cache = {}


def f32r(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def coefficients(p, v, a, origin, radius):
    """c[..., 0:5], lowest order first, in the kernels' order of operations (kf_aux.hpp sphere_query_values): plain double
    arithmetic, left to right, nothing fused."""
    q = p - origin
    px, py, pz = q[..., 0], q[..., 1], q[..., 2]
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    c4 = 0.25 * (ax * ax + ay * ay + az * az)
    c3 = vx * ax + vy * ay + vz * az
    c2 = vx * vx + vy * vy + vz * vz + px * ax + py * ay + pz * az
    c1 = 2 * (px * vx + py * vy + pz * vz)
    c0 = px * px + py * py + pz * pz - radius * radius
    return np.stack([c0, c1, c2, c3, c4], -1)


class Cases:
    """The fixture, for the f64 inputs or for the inputs rounded to f32 (reference results of that set)."""

    def __init__(self, dtype):
        z = np.load(FIXTURE)
        rd = f32r if dtype == "f32" else (lambda x: np.array(x, dtype=np.float64))
        s = "" if dtype == "f64" else "32"
        self.dtype = dtype
        self.p, self.v, self.a = rd(z["p"]), rd(z["v"]), rd(z["a"])
        self.origin, self.radius, self.scene = z["origin"], z["radius"], z["scene"]
        self.family_names = [str(n) for n in z["family_names"]]
        self.family = z["family"]
        self.delta, self.pos, self.m = z["delta" + s], z["pos" + s], z["m" + s]
        self.roots = dict(zip(z["unclear" + s].tolist(), z["roots" + s][..., 0] + 1j * z["roots" + s][..., 1]))
        self.c = coefficients(self.p, self.v, self.a, self.origin, self.radius)
        self.n = len(self.delta)
        self.clear = self.m > TAU
        assert sorted(self.roots) == np.nonzero(~self.clear)[0].tolist()
        # (origin, radius) of every scene: a kernel launch takes one sphere
        self.scenes = [(self.origin[self.scene == k][0], float(self.radius[self.scene == k][0])) for k in range(int(self.scene.max()) + 1)]

    def of(self, name):
        return self.family == self.family_names.index(name)


def cases(dtype="f64"):
    if ("cases", dtype) not in _cache:
        _cache[("cases", dtype)] = Cases(dtype)
    return _cache[("cases", dtype)]


def pose6(x3):
    """[n, 3] -> the [n, 7] / [n, 6] rows init_batch takes (identity orientation, no angular part)"""
    n = len(x3)
    return np.concatenate([x3, np.tile([0, 0, 0, 1.0], (n, 1))], 1), np.concatenate([x3, np.zeros((n, 3))], 1)


def host_solver(c, tmpdir):
    """te_quartic.hpp compiled with g++ (TE_QUARTIC_HOST) over the quartics c [n, 5]: (quartic_sturm_classify, first_crossing_quartic)"""
    exe, fin, fout = (os.path.join(str(tmpdir), f) for f in ("quartic_cases_host", "quartics.bin", "solved.bin"))
    src = os.path.join(ROOT, "tests", "host", "quartic_cases_host.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, src])
    np.ascontiguousarray(c, dtype=np.float64).tofile(fin)
    subprocess.check_call([exe, fin, fout], timeout=300)
    out = np.fromfile(fout).reshape(-1, 2)
    assert len(out) == len(c)
    return out[:, 0].astype(int), out[:, 1]


def oracle_answers(models, cs):
    """The project's oracle in the precision of the case set: uniform-acceleration targets straight after creation, queried at
    their own time with the sphere of their scene.  (delta [n], position [n, 3])"""
    key = ("oracle", cs.dtype)
    if key not in _cache:
        m = models["uniform_acceleration"]
        p0, _ = pose6(cs.p)
        orc = oracle.OracleBatch(m["model"], m["Q"], m["R"], m["P"], p0, 0.004, 0.0, pose6(cs.v)[1], pose6(cs.a)[1], dtype=cs.dtype)
        delta, pos = np.full(cs.n, np.nan), np.full((cs.n, 3), np.nan)
        for k, (origin, radius) in enumerate(cs.scenes):
            _, pose, d = orc.intersection_pose(0.0, origin, radius)
            sel = cs.scene == k
            delta[sel], pos[sel] = d[sel], pose[sel, :3]
        _cache[key] = (delta, pos)
    return _cache[key]


def unit(cs, eps):
    """8 eps |want| / min(1, m) per case: what a root's value is measured in"""
    return 8 * eps * np.abs(cs.delta) / np.minimum(1.0, np.maximum(cs.m, TINY))


def oracle_error(models, cs):
    """per family: (largest |d_oracle - want|, the largest of it in units of unit(cs, 2^-52)) over the clear hits"""
    key = ("oracle error", cs.dtype)
    if key not in _cache:
        d, _ = oracle_answers(models, cs)
        u = unit(cs, EPS["f64"])
        out = {}
        for f, name in enumerate(cs.family_names):
            sel = (cs.family == f) & cs.clear & (cs.delta > 0) & (d > -1)
            err = np.abs(d[sel] - cs.delta[sel])
            out[name] = (float(err.max()), float((err / u[sel]).max())) if sel.any() else (0.0, 0.0)
        _cache[key] = out
    return _cache[key]


def _residual_ok(c, d):
    c, d = np.asarray(c, dtype=np.longdouble), np.longdouble(d)
    val, mag = np.longdouble(0), np.longdouble(0)
    for k in range(4, -1, -1):
        val, mag = val * d + c[k], mag * d + abs(c[k])
    return abs(val) <= 64 * 2.0 ** -53 * mag


def _clear_real(z, j):
    """root j is real (the reference's threshold) and further than TAU, relatively, from every other root"""
    return abs(z[j].imag) < 1e-10 and all(abs(z[i] - z[j]) > TAU * max(abs(z[i]), abs(z[j])) for i in range(len(z)) if i != j)


def _unclear_ok(cs, i, d):
    """the rule for a case with m <= TAU; returns None or what is wrong"""
    z = cs.roots[i]
    clear = [z[j].real for j in range(len(z)) if _clear_real(z, j)]
    if d == -1:
        real = [r.real for r in z if abs(r.imag) < 1e-10]
        if real and min(real) >= 0 and min(real) in clear:
            return "-1, but the leftmost real root %.17g is clear" % min(real)
        return None
    if not d >= 0:
        return "neither -1 nor a time"
    if not any(abs(r.imag) <= TAU * abs(r) and abs(d - r.real) <= TAU * max(abs(d), TINY) for r in z):
        return "not within TAU of a root that is real within TAU"
    if not _residual_ok(cs.c[i], d):
        return "the residual is not rounding noise"
    if any(r < d - TAU * max(abs(d), abs(r)) for r in clear):
        return "a clear real root lies to its left"
    return None


def accept(tag, models, cs, delta, pos):
    """The acceptance rule (module docstring) for one solver's answers to every case: delta [n], pos [n, 3]."""
    delta, pos = np.asarray(delta, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    assert delta.shape == (cs.n,) and pos.shape == (cs.n, 3)
    assert np.isfinite(delta).all() and np.isfinite(pos).all(), (tag, "NaN or infinity", np.nonzero(~np.isfinite(delta))[0][:10])
    err_o = oracle_error(models, cs)
    want, clear, hit = cs.delta, cs.clear, cs.delta > -1
    bad = np.nonzero(clear & ((delta > -1) != hit))[0]
    assert len(bad) == 0, "%s: %d clear cases classified wrongly, first %s" % (tag, len(bad), [(int(i), cs.family_names[cs.family[i]], delta[i], want[i], cs.m[i]) for i in bad[:5]])
    miss = clear & ~hit
    assert (delta[miss] == -1).all() and (pos[miss] == 0).all(), (tag, "a miss is -1 with the identity pose")
    on_surface = clear & (cs.c[:, 0] == 0)
    assert (delta[on_surface] == want[on_surface]).all(), (tag, "c0 == 0", np.nonzero(on_surface & (delta != want))[0][:10])
    u64, uT = unit(cs, EPS["f64"]), unit(cs, EPS[cs.dtype])
    nv, na, npos = (np.linalg.norm(x, axis=1) for x in (cs.v, cs.a, cs.p))
    for f, name in enumerate(cs.family_names):
        sel = (cs.family == f) & clear & hit
        if sel.any():
            ko = K * np.minimum(err_o[name][0], err_o[name][1] * u64[sel])
            err = np.abs(delta[sel] - want[sel])
            perr = np.abs(pos[sel] - cs.pos[sel]).max(axis=1)
            pbound = (ko + uT[sel]) * (nv[sel] + na[sel] * want[sel]) + 8 * EPS[cs.dtype] * np.maximum(1.0, npos[sel])
            with np.errstate(divide="ignore", invalid="ignore"):
                r_k = np.where(err > 0, err / u64[sel], 0.0).max()
            print("[quartic] %-34s %-3s %-18s %4d clear hits  worst |d delta| / unit: solver %8.3f  oracle %8.3f   position / bound %6.3f"
                  % (tag, cs.dtype, name, sel.sum(), r_k, err_o[name][1], (perr / pbound).max()))
            w = np.nonzero(sel)[0][err > ko + u64[sel]]
            assert len(w) == 0, "%s %s: %d crossing times off, first %s" % (tag, name, len(w), [(int(i), delta[i], want[i], cs.m[i]) for i in w[:5]])
            w = np.nonzero(sel)[0][perr > pbound]
            assert len(w) == 0, "%s %s: %d positions off, first %s" % (tag, name, len(w), [(int(i), pos[i].tolist(), cs.pos[i].tolist()) for i in w[:5]])
    wrong = [(i, cs.family_names[cs.family[i]], delta[i], why) for i in np.nonzero(~clear)[0] for why in [_unclear_ok(cs, int(i), delta[i])] if why]
    assert not wrong, "%s: %d unclear cases, first %s" % (tag, len(wrong), wrong[:5])
    # an unclear case's position is the trajectory at the time it returns (or the identity pose)
    for i in np.nonzero(~clear)[0]:
        d = delta[i]
        traj = cs.p[i] + cs.v[i] * d + 0.5 * cs.a[i] * d * d if d > -1 else np.zeros(3)
        mag = npos[i] + nv[i] * d + na[i] * d * d if d > -1 else 0.0
        assert np.abs(pos[i] - traj).max() <= 8 * EPS[cs.dtype] * mag, (tag, "unclear case %d: position" % i, pos[i], traj)


# ---- the fixture's own conditions (asserted by the generator too) --------------------------------------------------------------
def fixture_conditions(cs, cls):
    """cs: a case set; cls: the host-compiled quartic_sturm_classify of its quartics.  Prints the counts."""
    names = cs.family_names
    hit = cs.delta > -1
    print("%-18s %6s %6s %6s %8s %10s %14s" % ("family (%s)" % cs.dtype, "cases", "hits", "misses", "unclear", "long road", "... with d > 0"))
    for f, name in enumerate(names):
        s = cs.family == f
        print("%-18s %6d %6d %6d %8d %10d %14d" % (name, s.sum(), (s & cs.clear & hit).sum(), (s & cs.clear & ~hit).sum(), (s & ~cs.clear).sum(),
                                                 (s & (cls == 0)).sum(), (s & (cls == 0) & (cs.delta > 0)).sum()))
    long_road = cls == 0
    print("long road %d of %d, with a crossing > 0: %d" % (long_road.sum(), cs.n, (long_road & (cs.delta > 0)).sum()))
    assert long_road.sum() >= 500 and (long_road & (cs.delta > 0)).sum() >= 100
    s = cs.of("closest approach")
    assert (s & long_road & (cs.delta > 0)).sum() >= 50
    assert (cs.c[cs.of("on the surface"), 0] == 0).sum() >= 100 and (cs.c[s, 1] == 0).sum() >= 100      # exact zeros, as constructed
    for f, name in enumerate(names):
        s = cs.family == f
        share = (s & ~cs.clear).sum() / s.sum()
        if name == UNCLEAR_FAMILY:
            # (rounding the inputs to f32 moves the path by 1e-7 R: in that set the family is grazing at 1e-7, and clear)
            assert share >= 0.5 or cs.dtype == "f32", (name, share)
            continue
        assert share <= 0.05, (name, share)
        if name == "semantic singles":
            continue
        # tangent is grazing's sub-family: its clear cases count with grazing's
        s = s | (cs.of(UNCLEAR_FAMILY) if name == "grazing" else False)
        assert (s & cs.clear & ~hit).sum() >= 20, (name, "misses")
        if name == "started inside":
            # p(0) = c0 < 0 < c4: the quartic has a negative root, the answer is -1 whatever the motion -- no hit can be drawn
            assert (cs.c[s, 0] < 0).all() and not (s & hit).any()
            continue
        assert (s & cs.clear & hit).sum() >= 20, (name, "hits")
    single = cs.of("semantic singles")
    assert (cs.delta[single] == -1).all()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("quartic_host")
    return {dt: host_solver(cases(dt).c, d) for dt in ("f64", "f32")}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fixture_conditions(host, dtype):
    cs = cases(dtype)
    assert os.path.getsize(FIXTURE) <= 1 << 20
    assert 2000 <= cs.n <= 4500
    fixture_conditions(cs, host[dtype][0])
    if dtype == "f64":
        # lengths scaled by a power of two scale every coefficient by a power of two: the same roots, to the bit
        base = np.nonzero(cs.of("configs[4] shape"))[0]
        for name in ("lengths 2^-20", "lengths 2^+20"):
            s = np.nonzero(cs.of(name))[0]
            assert np.array_equal(cs.delta[s], cs.delta[base[:len(s)]]) and np.array_equal(cs.m[s], cs.m[base[:len(s)]])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_oracle_passes_the_rule(models, dtype):
    cs = cases(dtype)
    accept("oracle", models, cs, *oracle_answers(models, cs))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_compiled_solver_passes_the_rule(models, host, dtype):
    """te_quartic.hpp with exact division and std::cbrt; the position is the trajectory at the returned time, in double."""
    cs = cases(dtype)
    d = host[dtype][1]
    t = np.where(d > -1, d, 0.0)[:, None]
    pos = np.where(d[:, None] > -1, cs.p + cs.v * t + 0.5 * cs.a * t * t, 0.0)
    if dtype == "f32":     # the f32 kernels evaluate the pose in f32 at the f32 time
        t32 = t.astype(np.float32)
        p32 = cs.p.astype(np.float32) + cs.v.astype(np.float32) * t32 + np.float32(0.5) * cs.a.astype(np.float32) * t32 * t32
        pos = np.where(d[:, None] > -1, p32.astype(np.float64), 0.0)
    accept("te_quartic.hpp on the host", models, cs, d, pos)


def test_oracle_deflates_exact_zero_roots():
    """orc_poly_roots with a zero constant term: the root 0 comes out exactly (as often as x divides the polynomial) and the others
    are the quotient's; lowest_real_root no longer hangs on the sign of a root of size 1e-89."""
    assert oracle.poly_roots([0.0, 3.0]).tolist() == [0]
    assert oracle.poly_roots([0.0, 0.0, 1.0]).tolist() == [0, 0]
    z = oracle.poly_roots([0.0, 0.0, -2.0, 1.0])
    assert z[:2].tolist() == [0, 0] and abs(z[2] - 2) <= 1e-15
    z = oracle.poly_roots([0.0, -6.0, 11.0, -6.0, 1.0])                   # x (x - 1)(x - 2)(x - 3)
    assert z[0] == 0 and np.abs(np.sort(z[1:].real) - [1, 2, 3]).max() <= 1e-14 and np.abs(z.imag).max() <= 1e-14
    assert oracle.lowest_real_root([0.0, -6.0, 11.0, -6.0, 1.0]) == 0.0
    assert abs(oracle.lowest_real_root([0.0, 6.0, 11.0, 6.0, 1.0]) + 3) <= 1e-14     # x (x + 1)(x + 2)(x + 3)
    assert len(oracle.poly_roots([0.0, 0.0, 0.0])) == 0
