#!/usr/bin/env python3
"""Hard sphere scenes for the intersection quartic, with 50-digit answers (mpmath), for tests/test_quartic_cases.py and
tests/test_gpu_quartic_cases.py (the acceptance rule is stated there).

    python tests/golden/make_quartic_cases.py        ->  tests/golden/quartic_cases.npz

A case is a uniform-acceleration target straight after its creation (state = [p v a] exactly) and a sphere (origin, radius).
Its reference: the quartic's five coefficients formed from the DOUBLE inputs in the kernels' order of operations (plain double,
left to right: test_quartic_cases.coefficients), the roots of that quartic by mpmath.polyroots at 50 digits, and the reference's
selection rule (as make_highprec_kat.py: |imag| < 1e-10 is real; the smallest real part; none, or a negative one, or a zero
leading coefficient -> -1).  c0 == 0 exactly is deflated by hand: 0 is a root and the others are the cubic's; -1 if the cubic has a
negative real root, otherwise 0.0.  Stored per case: p, v, a, origin, radius, scene (cases of one scene share the sphere: one
kernel launch), family, and twice -- for the inputs as they are and for the inputs rounded to f32 -- delta, the position at the
crossing, and the LOCAL margin m (the smallest |Im z| / |z| over the non-real roots and gap / max(|r_j|, |r_j+1|) over neighbouring
real roots; the four roots themselves where m <= 2^-20).

The conditions the families must meet (hits and misses in every family, how many quartics take the solver's long road, how many
cases are unclear) are asserted here and again by tests/test_quartic_cases.py::test_fixture_conditions.
"""
import os
import sys
import tempfile

import numpy as np
from mpmath import mp, mpf, polyroots

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_quartic_cases as tq  # noqa: E402

mp.dps = 50
SCENES = [(np.zeros(3), 1.0), (np.zeros(3), 4.5), (np.array([0.25, -0.5, 0.125]), 1.5), (np.zeros(3), 13.0),
          (np.zeros(3), 13.0 * 2.0 ** -20), (np.zeros(3), 13.0 * 2.0 ** 20), (np.zeros(3), 2.0 ** -20), (np.zeros(3), 2.0 ** 20)]


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def reference(p, v, a, origin, radius):
    """(delta, position [3], m, roots [4, 2]) of one case, doubles"""
    c = [mpf(float(x)) for x in tq.coefficients(p, v, a, origin, radius)]
    if c[4] == 0:
        return -1.0, np.zeros(3), 1.0, np.zeros((4, 2))
    if c[0] == 0:
        roots = [mp.mpc(0)] + list(polyroots([c[4], c[3], c[2], c[1]], maxsteps=2000, extraprec=1000))
    else:
        roots = list(polyroots(c[::-1], maxsteps=2000, extraprec=1000))
    real = sorted(r.real for r in roots if abs(r.imag) < mpf("1e-10"))
    if c[0] == 0:
        delta = mpf(-1) if any(r < 0 for r in real) else mpf(0)
    else:
        delta = real[0] if real and real[0] >= 0 else mpf(-1)
    terms = [abs(r.imag) / abs(r) for r in roots if abs(r.imag) >= mpf("1e-10")]
    terms += [(real[j + 1] - real[j]) / max(abs(real[j]), abs(real[j + 1])) if max(abs(real[j]), abs(real[j + 1])) > 0 else mpf(0)
              for j in range(len(real) - 1)]
    pos = [float(mpf(float(p[i])) + mpf(float(v[i])) * delta + mpf("0.5") * mpf(float(a[i])) * delta * delta) for i in range(3)] if delta >= 0 else [0.0] * 3
    return float(delta), np.array(pos), float(min(terms)), np.array([[float(r.real), float(r.imag)] for r in roots])


def families(rng):
    """[(family, scene, p, v, a)] with p, v, a [n, 3]"""
    out = []

    def aimed(p, origin, speed, spread):       # every other target flies at the sphere, so that a family has crossings
        d = origin - p
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d * speed[:, None] * (1 + spread * rng.normal(size=p.shape))

    # the host test's scene (p in [-10, 10]^3, v ~ 3 N, a ~ asc N), the acceleration's scale swept over 14 decades
    for asc in (1e2, 1.0, 1e-3, 1e-6, 1e-9, 1e-12):
        for scene in (1, 2):
            n = 30
            p = rng.uniform(-10, 10, (n, 3))
            v = 3 * rng.normal(size=(n, 3))
            v[::2] = aimed(p[::2], SCENES[scene][0], rng.uniform(1, 6, n)[::2], 0.1)
            out.append(("acceleration sweep", scene, p, v, asc * rng.normal(size=(n, 3))))
    # BASELINE configs[4]: |p| ~ 6, |v| ~ 0.2, |a| ~ 1e-2 .. 1e-3, R = 1; and the same cases with every length scaled
    n = 300
    p = 6 * rng.normal(size=(n, 3))
    v = 0.2 * rng.normal(size=(n, 3))
    v[::2] = aimed(p[::2], np.zeros(3), rng.uniform(0.1, 0.5, n)[::2], 0.04)
    a = np.where(np.arange(n)[:, None] % 2 == 1, 1e-2, 1e-3) * rng.normal(size=(n, 3))
    out.append(("configs[4] shape", 0, p, v, a))
    for name, scene, s in (("lengths 2^-20", 6, 2.0 ** -20), ("lengths 2^+20", 7, 2.0 ** 20)):
        out.append((name, scene, p[:150] * s, v[:150] * s, a[:150] * s))

    # grazing (the host test's construction): a straight line through n d, d = R (1 + eps), orthogonal to n, a small acceleration
    def grazing(n, eps, asc):
        nrm = unit(rng, n)
        t = rng.normal(size=(n, 3))
        t -= (t * nrm).sum(1, keepdims=True) * nrm
        s0 = rng.choice([-1.0, 1.0], n) * (1 + 10 * rng.uniform(size=n))
        return nrm * (1 + eps)[:, None] - t * s0[:, None], t, asc[:, None] * rng.normal(size=(n, 3))
    n = 300
    out.append(("grazing", 0, *grazing(n, rng.choice([-1.0, 1.0], n) * 10.0 ** -rng.uniform(3, 12, n), 10.0 ** rng.uniform(-8, -2, n))))
    n = 120
    eps = rng.choice([-1.0, 1.0], n) * 10.0 ** -rng.uniform(13, 17, n)
    eps[::6] = 0.0
    out.append(("tangent", 0, *grazing(n, eps, 10.0 ** -rng.uniform(12, 15, n))))
    # on the surface: c0 == 0 exactly from Pythagorean quadruples (3, 4, 12 | 13), (0, 5, 12 | 13) scaled by 2^k ...
    for scene, k in ((3, 0), (4, -20), (5, 20)):
        n = 100
        base = np.where(rng.uniform(size=(n, 1)) < 0.7, [3.0, 4.0, 12.0], [0.0, 5.0, 12.0])
        p = np.stack([rng.permutation(b) for b in base]) * rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** k
        v = rng.normal(size=(n, 3)) * 3 * 2.0 ** k
        v[::2] = aimed(p[::2], np.zeros(3), rng.uniform(1, 6, n)[::2] * 2.0 ** k, 0.3)
        out.append(("on the surface", scene, p, v, 10.0 ** rng.uniform(-3, 1, (n, 1)) * rng.normal(size=(n, 3)) * 2.0 ** k))
    # ... and |p| = R (1 +- 1e-3 .. 1e-16)
    for scene in (0, 3):
        n = 100
        R = SCENES[scene][1]
        p = unit(rng, n) * (R * (1 + rng.choice([-1.0, 1.0], n) * 10.0 ** -rng.uniform(3, 16, n)))[:, None]
        v = rng.normal(size=(n, 3)) * R
        v[::2] = aimed(p[::2], np.zeros(3), rng.uniform(0.3, 2, n)[::2] * R, 0.3)
        out.append(("on the surface", scene, p, v, 10.0 ** rng.uniform(-3, 0, (n, 1)) * rng.normal(size=(n, 3)) * R))
    # closest approach now: c1 == 0 exactly (p on one axis, v in the orthogonal plane, entries multiples of 1/8), and p orthogonal
    # to v only to rounding.  An acceleration that merely points back at the sphere gives a path that is symmetric in time about
    # now: it fell out of the sphere as it will fall into it, the leftmost root is negative and the answer -1.  A crossing AHEAD
    # only needs the target to come back: a = -k v^ - g p^ brakes the tangential motion (speed s), which returns to the
    # foot point at t* = 2 s / k, while the radial distance r - g t^2 / 2 is inside the sphere at t* for g = (r + u R) k^2 / (2 s^2),
    # |u| < 1; with k = s^2 / (w R) the path before now was further than 4 w R out when it was level with the sphere.
    def back_at_the_sphere(p, v, R):
        n = len(p)
        r, s = np.linalg.norm(p, axis=1), np.linalg.norm(v, axis=1)
        k = s * s / (R * rng.uniform(0.5, 2, n))
        g = (r + R * rng.uniform(-0.8, 0.8, n)) * k * k / (2 * s * s)
        a = -k[:, None] * v / s[:, None] - g[:, None] * p / r[:, None]
        return a * (1 + 0.01 * rng.normal(size=(n, 3)))
    for scene in (0, 1):
        n = 200
        R = SCENES[scene][1]
        axis = rng.integers(0, 3, n)
        p, v = np.zeros((n, 3)), np.zeros((n, 3))
        p[np.arange(n), axis] = np.ceil(8 * R * rng.uniform(1.05, 4, n)) / 8 * rng.choice([-1.0, 1.0], n)
        for j in (1, 2):
            v[np.arange(n), (axis + j) % 3] = rng.integers(-24, 25, n) / 8
        v[np.arange(n), (axis + 1) % 3] += np.where((v == 0).all(1), 0.5, 0.0)      # (no target at rest)
        a = 10.0 ** rng.uniform(-3, 0, (n, 1)) * rng.normal(size=(n, 3))
        a[::2] = back_at_the_sphere(p[::2], v[::2], R)
        out.append(("closest approach", scene, p, v, a))
    n = 200
    p = unit(rng, n) * rng.uniform(1.05, 6, (n, 1))
    v = rng.normal(size=(n, 3))
    v -= (v * p).sum(1, keepdims=True) / (p * p).sum(1, keepdims=True) * p
    a = 10.0 ** rng.uniform(-3, 0, (n, 1)) * rng.normal(size=(n, 3))
    a[::2] = back_at_the_sphere(p[::2], v[::2], 1.0)
    out.append(("closest approach", 0, p, v, a))
    # radial: v and a parallel to p, inbound and outbound
    for scene in (0, 1):
        n = 100
        d = unit(rng, n)
        p = d * (SCENES[scene][1] * rng.uniform(1.1, 8, n))[:, None]
        out.append(("radial", scene, p, d * (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 5, n))[:, None],
                    d * (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 1, n))[:, None]))
    # started inside the sphere
    n = 150
    p = SCENES[2][0] + unit(rng, n) * rng.uniform(0.05, 1.45, (n, 1))
    out.append(("started inside", 2, p, 2 * rng.normal(size=(n, 3)), 10.0 ** rng.uniform(-6, 1, (n, 1)) * rng.normal(size=(n, 3))))
    # semantics: zero acceleration -> -1 (the leading coefficient is zero), flying away
    d = unit(rng, 8)
    p = SCENES[2][0] + d * rng.uniform(2, 9, (8, 1))
    v = -d * rng.uniform(1, 4, (8, 1))
    a = np.zeros((8, 3))
    v[4:], a[4:] = d[4:] * rng.uniform(1, 4, (4, 1)), d[4:] * rng.uniform(0.5, 2, (4, 1))
    out.append(("semantic singles", 2, p, v, a))
    return out


def main():
    rng = np.random.default_rng(20250611)
    fams = families(rng)
    names = []
    for f in fams:
        if f[0] not in names:
            names.append(f[0])
    P, V, A = (np.concatenate([f[k] for f in fams]) for k in (2, 3, 4))
    scene = np.concatenate([np.full(len(f[2]), f[1]) for f in fams]).astype(np.int8)
    family = np.concatenate([np.full(len(f[2]), names.index(f[0])) for f in fams]).astype(np.int8)
    origin = np.stack([SCENES[s][0] for s in scene])
    radius = np.array([SCENES[s][1] for s in scene])
    out = dict(p=P, v=V, a=A, origin=origin, radius=radius, scene=scene, family=family, family_names=np.array(names))
    for sfx, rd in (("", lambda x: x), ("32", tq.f32r)):
        res = [reference(rd(P[i]), rd(V[i]), rd(A[i]), origin[i], radius[i]) for i in range(len(P))]
        m = np.array([r[2] for r in res])
        unclear = np.nonzero(~(m > tq.TAU))[0]
        out.update({"delta" + sfx: np.array([r[0] for r in res]), "pos" + sfx: np.stack([r[1] for r in res]), "m" + sfx: m,
                    "unclear" + sfx: unclear.astype(np.int32), "roots" + sfx: np.array([res[i][3] for i in unclear]).reshape(-1, 4, 2)})
    np.savez_compressed(tq.FIXTURE, **out)
    print("%d cases, %d bytes" % (len(P), os.path.getsize(tq.FIXTURE)))
    with tempfile.TemporaryDirectory() as tmp:
        for dtype in ("f64", "f32"):
            cs = tq.Cases(dtype)
            tq.fixture_conditions(cs, tq.host_solver(cs.c, tmp)[0])


if __name__ == "__main__":
    main()
