"""The attitude fixture (tests/golden/make_attitude_kat.py -> tests/golden/attitude_kat.npz) as the tests of
tests/test_attitude_kat.py and tests/test_gpu_attitude_kat.py read it: the expected rows of every view, their groups, and the
error of a set of rows per group.

A group is view x branch of the matrix -> quaternion rule ("now/i1", "at/trace", "ticks/i0", ...) or "gimbal"; every group is
split into its STRICT rows (compared as they are, the quaternion's sign included) and the rest (name + "~": compared as
rotations, q or -q whichever is nearer).  The error of a row is max |got - want| / max(1, |want|) over its entries, the error of
a group the maximum over its rows."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ANGULAR = ("angular_rates", "angular_velocities")
CONTROLS = ("uniform_velocity", "uniform_acceleration")
TOLERANCES = os.path.join(ROOT, "profiles", "attitude_kat_tolerances.txt")

_kat = {}


def load():
    if not _kat:
        with np.load(os.path.join(HERE, "golden", "attitude_kat.npz")) as z:
            _kat.update({k: (z[k].astype(np.float64) if z[k].dtype == np.float32 else z[k]) for k in z.files})
        for a in _kat.values():
            a.setflags(write=False)
    return _kat


class Model:
    """one model's inputs and expected rows"""

    def __init__(self, name):
        k = load()
        g = lambda key: k["%s_%s" % (key, name)]  # noqa: E731
        self.name, self.angular = name, name in ANGULAR
        self.dt, self.offsets, self.group_names = float(k["dt"]), k["offsets"], [str(s) for s in k["groups"]]
        self.p0, self.v0, self.a0, self.set = g("p0"), g("v0"), g("a0"), g("set")
        self.n = len(self.p0)
        self.offset_of = np.arange(self.n) % len(self.offsets)
        self.now = np.concatenate([g("now_pos"), g("now_quat"), g("now_twl"), g("now_twa"), g("now_acc")], 1)          # [n, 19]
        self.at = np.concatenate([g("at_pos"), g("at_quat"), g("at_twl"), g("at_twa"), g("now_acc")], 1)              # [n, 19] (acc: as now)
        if self.angular:
            self.strict_now, self.group_now, self.group_at = g("strict_now"), g("group_now"), g("group_at")
            self.branch_now, self.d_now = g("branch_now"), g("d_now")
            self.tick_cases = g("tick_cases").astype(np.int64)
            self.tick_pose = np.concatenate([g("tick_pos"), g("tick_quat")], 2)                                         # [3, M, 7]
            self.x_k = np.insert(g("xk_rest"), [3, 3, 3], 0.0, axis=2)
            self.x_k[:, :, 3:6] = g("xk_rpy")                                                                         # [3, M, ns]
            self.strict_k, self.group_k, self.branch_k, self.d_k = g("strict_k"), g("group_k"), g("branch_k"), g("d_k")
        else:       # the controls: one group per view, every row strict
            self.strict_now = np.ones(self.n, bool)
            self.group_now, self.group_at = np.zeros(self.n, np.int8), np.full(self.n, 4, np.int8)
            self.tick_cases = np.zeros(0, np.int64)
        self.gimbal = self.set == 3

    def inputs(self, cases=None):
        """p0, v0, a0 of `cases` (all of them by default); every value is an f32, so no precision rounds them"""
        c = slice(None) if cases is None else cases
        return self.p0[c].copy(), self.v0[c].copy(), self.a0[c].copy()


def _unsign(q, ref):
    flip = (np.abs(q - ref).max(1) > np.abs(q + ref).max(1))[:, None]
    return np.where(flip, -q, q)


def row_errors(got, want, strict):
    """per row: max |got - want| / max(1, |want|); columns 3:7 are a quaternion, up to sign where the row is not strict"""
    got = np.array(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    loose = ~np.asarray(strict)
    if loose.any():
        got[loose, 3:7] = _unsign(got[loose, 3:7], want[loose, 3:7])
    return (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max(axis=1)


def group_errors(m, view, got, rows=None, pose_only=False):
    """{group name (+ "~" for its rows that are not strict): error} of one view.  view "now" / "at": got [len(rows), 19] for the
    cases `rows` (all by default; of "at", those whose own offset was asked); view ("ticks", k): got [M, 7], tick k + 1 of
    tick_cases.  The gimbal set is held on pose7 of "now" only.  pose_only: got has pose7 only (the pose streams)."""
    out = {}
    if isinstance(view, tuple):
        k = view[1]
        want, strict, group = m.tick_pose[k], m.strict_k[k], m.group_k[k]
        if rows is not None:
            want, strict, group = want[rows], strict[rows], group[rows]
        err = row_errors(got, want, strict)
    else:
        rows = np.arange(m.n) if rows is None else np.asarray(rows)
        want = (m.now if view == "now" else m.at)[rows]
        strict, group = m.strict_now[rows], (m.group_now if view == "now" else m.group_at)[rows]
        got = np.asarray(got)
        width = 7 if pose_only else 19
        err = row_errors(got[:, :width], want[:, :width], strict)
        gim = m.gimbal[rows]
        if gim.any():
            err[gim] = row_errors(got[gim, :7], want[gim, :7], strict[gim]) if view == "now" else 0.0
    for g in np.unique(group):
        if g < 0:
            continue
        for s, mark in ((True, ""), (False, "~")):
            sel = (group == g) & (strict == s)
            if sel.any():
                out[m.group_names[g] + mark] = float(err[sel].max())
    return out


def merge(into, errs):
    for k, v in errs.items():
        into[k] = max(into.get(k, 0.0), v)
    return into


_oracle_cache = {}


def oracle_outputs(oracle, models, name, dtype):
    """the C oracle of precision `dtype` over every view of model `name` (computed once): dict(now [n,19], at [n,19] -- every
    case at its own offset --, ticks [3, M, 7])"""
    if (name, dtype) in _oracle_cache:
        return _oracle_cache[(name, dtype)]
    m, mod = Model(name), models[name]
    p0, v0, a0 = m.inputs()
    orc = oracle.OracleBatch(mod["model"], mod["Q"], mod["R"], mod["P"], p0, m.dt, 0.0, v0, a0, dtype=dtype)
    out = dict(now=np.concatenate([orc.pose(), orc.twist(), orc.acceleration()], 1), at=np.zeros((m.n, 19)),
               ticks=np.zeros((3, len(m.tick_cases), 7)))
    for o, off in enumerate(m.offsets):
        rows = m.offset_of == o
        out["at"][rows] = np.concatenate([orc.pose_at(off), orc.twist_at(off), orc.acceleration_at(off)], 1)[rows]
    if len(m.tick_cases):
        p0, v0, a0 = m.inputs(cases=m.tick_cases)
        orc = oracle.OracleBatch(mod["model"], mod["Q"], mod["R"], mod["P"], p0, m.dt, 0.0, v0, a0, dtype=dtype)
        for k in range(3):
            orc.step(m.dt, None)
            out["ticks"][k] = orc.pose()
    for a in out.values():
        a.setflags(write=False)
    _oracle_cache[(name, dtype)] = out
    return out


def oracle_errors(oracle, models, name, dtype):
    """{group: error} of the oracle's outputs over every view"""
    m, out = Model(name), oracle_outputs(oracle, models, name, dtype)
    errs = merge(group_errors(m, "now", out["now"]), group_errors(m, "at", out["at"]))
    for k in range(3 if len(m.tick_cases) else 0):
        merge(errs, group_errors(m, ("ticks", k), out["ticks"][k]))
    return errs


def twin_errors(models, name):
    """oracle/np_twin.py (fp64) over every view: {group: error}"""
    from oracle import np_twin as tw
    m, mod = Model(name), models[name]
    errs = {}
    now, at = np.zeros((m.n, 19)), np.zeros((m.n, 19))
    ticks = np.zeros((3, len(m.tick_cases), 7))
    for i in range(m.n):
        t = tw.Target(mod["model"], mod["Q"], mod["R"], mod["P"], m.p0[i], m.dt, 0.0, m.v0[i], m.a0[i])
        off = float(m.offsets[m.offset_of[i]])
        now[i] = np.concatenate([t.pose(), t.twist, t.acceleration])
        at[i] = np.concatenate([t.pose_at(off), t.twist_at(off), t.acceleration])
        j = np.nonzero(m.tick_cases == i)[0]
        for k in range(3 if len(j) else 0):
            t.update(m.dt)
            ticks[k, j[0]] = t.pose()
    merge(errs, group_errors(m, "now", now))
    merge(errs, group_errors(m, "at", at))
    for k in range(3 if len(m.tick_cases) else 0):
        merge(errs, group_errors(m, ("ticks", k), ticks[k]))
    return errs


def read_ceilings():
    """{(model, precision, group): (measured, ceiling)} of the `cpu` lines of profiles/attitude_kat_tolerances.txt"""
    out = {}
    with open(TOLERANCES) as f:
        for line in f:
            w = line.split()
            if len(w) == 6 and w[0] == "cpu":
                out[(w[1], w[2], w[3])] = (float(w[4]), float(w[5]))
    return out


GPU_MARK = "# ---- MI355X"
ROUNDING = 2.0 ** -53


def ceiling(measured):
    """4 x the measured error; every result is handed over as a double, so an error below one rounding of it (an f80 oracle that
    rounds to the fixture's very double, exact arithmetic on the controls' grids) is measured as that rounding"""
    return 4.0 * max(measured, ROUNDING)


def write_tolerances():
    """python tests/attitude_kat_ref.py: measure the oracles and the twin against the fixture on this machine and rewrite the cpu
    lines of profiles/attitude_kat_tolerances.txt (what follows GPU_MARK is kept)."""
    import sys
    sys.path.insert(0, ROOT)
    import oracle
    models = {k: oracle.load_model_yaml(os.path.join(ROOT, "models", "model_%s_params.yaml" % k)) for k in ANGULAR + CONTROLS}
    tail = ""
    if os.path.exists(TOLERANCES):
        old = open(TOLERANCES).read()
        if GPU_MARK in old:
            tail = old[old.index(GPU_MARK):]
    lines = ["# Derived outputs against the 50-digit attitude fixture (tests/golden/attitude_kat.npz), per model, precision and group:",
             "# the CPU oracle's (f32 / f64 / f80) and the NumPy twin's worst error, max |got - want| / max(1, |want|) over a group's rows,",
             "# and the ceiling tests/test_attitude_kat.py holds them to: 4 x the measured error (libm differs between machines), a measured",
             "# error below 2^-53 counting as 2^-53 (every side hands its results over as doubles: one rounding is the least that shows).",
             "# group = view x branch of the matrix -> quaternion rule; name~ = its rows that are not strict (compared as rotations).",
             "# Regenerate: python tests/attitude_kat_ref.py",
             "#   model precision group measured ceiling"]
    for name in ANGULAR + CONTROLS:
        for prec in ("f32", "f64", "f80", "twin"):
            errs = twin_errors(models, name) if prec == "twin" else oracle_errors(oracle, models, name, prec)
            for g in sorted(errs):
                lines.append("cpu %s %s %s %.3e %.3e" % (name, prec, g, errs[g], ceiling(float("%.3e" % errs[g]))))
    with open(TOLERANCES, "w") as f:
        f.write("\n".join(lines) + "\n" + tail)
    print("\n".join(lines))


def append_gpu_table(log):
    """python tests/attitude_kat_ref.py LOG: the `[attitude]` rows of `pytest -m gpu -s tests/test_gpu_attitude_kat.py`, condensed
    to the worst row per (path, model, precision, group) over the layouts, offsets and ticks, replace what follows GPU_MARK."""
    import re
    worst, n = {}, 0
    for line in open(log):
        w = re.search(r"\[attitude\] (.*?)\s+(angular_\w+|uniform_\w+)\s+(f64|f32)\s+(\S+)\s+kernel (\S+)\s+faithful (\S+)\s+ratio\s+(\S+)", line)
        if not w:
            continue
        n += 1
        path = re.sub(r" (t1 \S+|tick \d)$", "", w.group(1))
        path = re.sub(r" (301shared|301|201|full|packed|classes|auto)\b", "", path)
        key = (path, w.group(2), w.group(3), w.group(4))
        row = (float(w.group(7)), float(w.group(5)), float(w.group(6)))
        if key not in worst or row > worst[key]:
            worst[key] = row
    head = open(TOLERANCES).read()
    if GPU_MARK in head:
        head = head[:head.index(GPU_MARK)]
    lines = [GPU_MARK + ": %d rows of tests/test_gpu_attitude_kat.py (every layout, offset and tick), the worst per path, model, precision and group;" % n,
             "# rule: kernel <= 8 x faithful + 8 eps, faithful = the same-precision CPU oracle on the same rows; ratio = kernel / max(faithful, 8 eps)",
             "#   path | model precision group kernel faithful ratio"]
    for key in sorted(worst):
        r = worst[key]
        lines.append("gpu %-36s | %s %s %s %.2e %.2e %.2f" % (key[0], key[1], key[2], key[3], r[1], r[2], r[0]))
    with open(TOLERANCES, "w") as f:
        f.write(head + "\n".join(lines) + "\n")
    print("%d rows, %d lines, worst ratio %.2f" % (n, len(worst), max(r[0] for r in worst.values())))


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:
        append_gpu_table(sys.argv[1])
    else:
        write_tolerances()
