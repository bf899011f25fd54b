#!/usr/bin/env python3
"""50-digit known answers for the derived outputs (pose7 / twist6 / acceleration6) over every attitude: all four branches of the
matrix -> quaternion rule, the quaternion's sign, the extrapolating getters at four offsets, predict-only ticks that carry the
angular-rates pitch past +-pi/2, the gimbal branches of the init conversion, omega = 0 and |omega| = 2^-40.

    python tests/golden/make_attitude_kat.py        ->  tests/golden/attitude_kat.npz

The formulas are those of tests/golden/make_highprec_kat.py (typed from the reference sources), imported, not retyped.  Every
input (p0 with a non-unit quaternion of either overall sign, v0, a0, dt, the offsets) is exactly f32-representable, so the one
fixture serves both precisions: all three sides of a comparison start from the same numbers.

Per angular model N = 457 targets ("cases"; 457 is neither a multiple of 64 nor of 10, the targets of a 6-lane tile), created at
t = 0 with (p0, v0, a0):
    set 0  the attitude grid   roll {0, +-1, 1.6, +-2.2, +-3.1} x pitch {0, +-0.7, +-1.5} x yaw {0, 0.4, +-1.3, +-2.6, +-3.1}
    set 1  random attitudes
    set 2  the cuts            roll or yaw = +-pi, a rotation by 120 degrees (trace = 0), by 180 degrees about (1,1,0), (0,1,1),
                               (1,-1,0) (the two largest diagonal entries tie): decided by rounding in any precision
    set 3  the gimbal set      |sin pitch| > 0.9999 at init, both signs
Views of a case:
    now    pose7 twist6 acc6 at the target's own time
    at     pose7 twist6 at t1 = OFFSETS[case % 4]: 0 (own time, through the extrapolating formulas), +1/16, -1/32, 2.5 s
    tick k pose7 and the state after k = 1, 2, 3 predict-only ticks of dt = 1/16 (every fourth case outside the gimbal set: tick_cases)
The gimbal set has the view `now` only, and of it pose7 only: with state pitch = +-pi/2 rot_to_rpy's roll is the atan2 of two
rounding residues.

Stored with every row: the branch taken (0 trace > 0, 1 i = 0, 2 i = 1, 3 i = 2), the decision values d_* on the way
    d[0]  |sin pitch| - 0.9999 of the init conversion                       (signed)
    d[1]  the least distance of an atan2 result of quat_to_rpy to +-pi
    d[2]  trace                                                             (signed)
    d[3]  the gap between the two largest diagonal entries where trace <= 0 (9 otherwise)
    d[4]  the least distance of an atan2 result (roll, yaw) of rot_to_rpy to +-pi
    d[5]  cos(state pitch); for tick k of the EKF, whose f divides by it, the one of least magnitude among the states 0 .. k   (signed)
(the tick rows store d[2:]; d[0] and d[1] are their case's)
and a group = view x branch (12 groups) or the gimbal set (group 12).  A row is STRICT when |d[0]|, d[1], |d[2]|, d[3], d[4] >= 1e-5
and |d[5]| >= 0.05: compared as it is, sign included.  The rest are compared as rotations (q up to sign)."""
import os
import sys

import numpy as np
from mpmath import mp, mpf, cos, atan2, matrix

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_highprec_kat import (outputs, quat_to_rpy, normalised, rpy_to_quat, quat_to_rot, rot_to_rpy,  # noqa: E402
                               transition_linear, ekf_f, rpy_quat, M_PI)

mp.dps = 50
N = 457
N_CONTROL = 37
N_GIMBAL = 26
DT = 0.0625
OFFSETS = np.array([0.0, 0.0625, -0.03125, 2.5])
TICKS = 3
TICK_EVERY, TICK_PHASE = 4, 1      # the cases that are ticked: every fourth one outside the gimbal set (the fixture's size)
ANGULAR = ("angular_rates", "angular_velocities")
MODELS = ANGULAR + ("uniform_velocity", "uniform_acceleration")      # the last two: a short control of the identity orientation and the offsets
SEED = 20261021
NS = {"uniform_velocity": 6, "uniform_acceleration": 9, "angular_rates": 18, "angular_velocities": 12}
BRANCHES = ["trace", "i0", "i1", "i2"]
VIEWS = ["now", "at", "ticks"]
GROUPS = ["%s/%s" % (v, b) for v in VIEWS for b in BRANCHES] + ["gimbal"]
MARGIN, MIN_COS = 1e-5, 0.05


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def grid(rng, lo, hi, step, size):
    """multiples of `step` in [lo, hi]: few significant bits, exact in f32 and in every sum the outputs form of them"""
    return np.round(rng.uniform(lo, hi, size) / step) * step


def attitudes(rng):
    """rpy [N,3] and the set of every case"""
    rolls = [0, 1, -1, 1.6, 2.2, -2.2, 3.1, -3.1]
    pitches = [0, 0.7, -0.7, 1.5, -1.5]
    yaws = [0, 0.4, 1.3, -1.3, 2.6, -2.6, 3.1, -3.1]
    rpy = [(r, p, y) for r in rolls for p in pitches for y in yaws]
    sets = [0] * len(rpy)
    pi = float(np.pi)
    cuts = [(pi, 0.3, 0.5), (-pi, -0.4, 1.0), (0.7, 0.2, pi), (-0.9, 0.5, -pi), (pi, 0.1, pi), (-pi, -0.2, -pi), (pi, 0.0, 0.0)]
    rpy += cuts
    sets += [2] * len(cuts)
    n_special = 4 + 3 + N_GIMBAL
    n_random = N - len(rpy) - n_special
    rpy += [(rng.uniform(-3.14, 3.14), rng.uniform(-1.45, 1.45), rng.uniform(-3.14, 3.14)) for _ in range(n_random)]
    sets += [1] * n_random
    quats = [None] * len(rpy)
    for k in range(4):          # trace = 0: a rotation by 120 degrees about a random axis (w = 1/2)
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        quats.append(np.concatenate([np.sqrt(0.75) * a, [0.5]])); rpy.append(None); sets.append(2)
    for a in ((1, 1, 0), (0, 1, 1), (1, -1, 0)):    # 180 degrees about a face diagonal: two diagonal entries tie ((1,0,1) is a gimbal attitude)
        quats.append(np.array(a + (0,), dtype=float)); rpy.append(None); sets.append(2)
    for k in range(N_GIMBAL):   # gimbal: |sin pitch| = cos(delta) > 0.9999 for delta < 0.01414; delta <= 0.012 keeps 2.8e-5 from the threshold
        sign = 1.0 if k % 2 == 0 else -1.0
        rpy.append((rng.uniform(-3, 3), sign * (np.pi / 2 - rng.uniform(0.0, 0.012)), rng.uniform(-3, 3))); sets.append(3)
        quats.append(None)
    out = np.zeros((N, 4))
    for i in range(N):
        q = np.array(rpy_quat(*rpy[i])) if rpy[i] is not None else quats[i]
        out[i] = q / np.linalg.norm(q)
    return out, np.array(sets, dtype=np.int8)


def make_inputs(model):
    rng = np.random.default_rng(SEED + MODELS.index(model))
    if model in ANGULAR:
        q, sets = attitudes(rng)
    else:                                           # the uniform models ignore the orientation of p0: any quaternion, identity out
        q, sets = rng.normal(size=(N_CONTROL, 4)), np.ones(N_CONTROL, dtype=np.int8)
    N = len(sets)
    order = rng.permutation(N)                      # the sets are spread over the batch, not stacked in tiles
    q, sets = q[order], sets[order]
    scale = rng.uniform(0.5, 2.0, N) * np.where(rng.random(N) < 0.5, -1.0, 1.0)      # non-unit, either overall sign
    p0 = np.concatenate([grid(rng, -8, 8, 2.0 ** -6, (N, 3)), f32(q * scale[:, None])], 1)
    v0 = np.concatenate([grid(rng, -2, 2, 2.0 ** -5, (N, 3)), np.zeros((N, 3))], 1)
    a0 = np.concatenate([grid(rng, -1, 1, 2.0 ** -5, (N, 3)), np.zeros((N, 3))], 1)
    if model == "angular_rates":                    # roll / yaw rates up to 1, pitch rates up to 3 rad/s: pitch passes +-pi/2 within three ticks
        v0[:, 3:] = np.stack([grid(rng, -1, 1, 2.0 ** -8, N), grid(rng, -3, 3, 2.0 ** -8, N), grid(rng, -1, 1, 2.0 ** -8, N)], 1)
        a0[:, 3:] = grid(rng, -0.5, 0.5, 2.0 ** -6, (N, 3))
        # the steep cases among those that are ticked move on towards +-pi/2 at 1 to 3 rad/s, and pass it
        qn = p0[:, 3:] / np.linalg.norm(p0[:, 3:], axis=1)[:, None]
        sp = -2 * (qn[:, 0] * qn[:, 2] - qn[:, 3] * qn[:, 1])
        steep = (np.abs(sp) > np.sin(1.3)) & (np.arange(N) % TICK_EVERY == TICK_PHASE)
        v0[steep, 4] = np.sign(sp[steep]) * grid(rng, 1, 3, 2.0 ** -8, steep.sum())
    elif model == "angular_velocities":
        w = grid(rng, -1.7, 1.7, 2.0 ** -8, (N, 3))                                   # |omega| up to 3 rad/s
        i = np.arange(N)
        w[i % 8 == 0] = 0.0                                                          # omega = 0 exactly
        tiny = i % 8 == 1
        w[tiny] = 0.0
        w[tiny, i[tiny] // 8 % 3] = np.where(i[tiny] % 16 == 1, 1.0, -1.0) * 2.0 ** -40   # |omega| = 2^-40
        # the EKF's f divides by cos(pitch): near +-pi/2 keep |omega| <= 0.25 so that three ticks stay 0.02 away in cos
        qn = p0[:, 3:] / np.linalg.norm(p0[:, 3:], axis=1)[:, None]
        sp = -2 * (qn[:, 0] * qn[:, 2] - qn[:, 3] * qn[:, 1])
        steep = np.abs(sp) > np.sin(1.3)
        w[steep] = np.round(w[steep] / 8 * 256) / 256
        v0[:, 3:] = w
        a0[:] = 0.0                                                                  # the model has no acceleration state
    else:
        a0[:, 3:] = 0.0
        if model == "uniform_velocity":
            a0[:] = 0.0
    for a in (p0, v0, a0):
        assert np.array_equal(f32(a), a)
    return p0, v0, a0, sets


def dist_pi(a):
    return min(abs(a - M_PI), abs(a + M_PI))


def init_state(model, p0, v0, a0):
    """x at t = 0 (the constructors), and d[0], d[1] of the conversion"""
    n = NS[model]
    x = [mpf(0)] * n
    for i in range(3):
        x[i] = mpf(p0[i])
    if model not in ANGULAR:
        for i in range(3):
            x[3 + i] = mpf(v0[i])
            if n == 9:
                x[6 + i] = mpf(a0[i])
        return x, mpf(9), mpf(9)
    q = normalised([mpf(v) for v in p0[3:7]])
    sp = -2 * (q[0] * q[2] - q[3] * q[1])
    rpy = quat_to_rpy(q)
    if abs(sp) > mpf("0.9999"):
        d1 = dist_pi(atan2(q[2], q[3]))
    else:
        d1 = min(dist_pi(rpy[0]), dist_pi(rpy[2]))
    for i in range(3):
        x[3 + i] = rpy[i]
    for i in range(6):
        x[6 + i] = mpf(v0[i])
        if n == 18:
            x[12 + i] = mpf(a0[i])
    return x, abs(sp) - mpf("0.9999"), d1


def decisions(x):
    """branch and d[2], d[3], d[4], cos(state pitch) of the orientation outputs of state x"""
    m = quat_to_rot(rpy_to_quat(list(x[3:6])))
    tr = m[0][0] + m[1][1] + m[2][2]
    diag = sorted([m[0][0], m[1][1], m[2][2]])
    if tr > 0:
        branch, gap = 0, mpf(9)
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        branch, gap = 1 + i, diag[2] - diag[1]
    r = rot_to_rpy(m)
    return branch, tr, gap, min(dist_pi(r[0]), dist_pi(r[2])), cos(x[4])


def is_strict(d):
    return bool(abs(d[0]) >= MARGIN and d[1] >= MARGIN and abs(d[2]) >= MARGIN and d[3] >= MARGIN and d[4] >= MARGIN and abs(d[5]) >= MIN_COS)


def fl(v):
    return [float(c) for c in v]


def pack(a):
    """f32 where that holds every value exactly (inputs, positions, linear twists), f64 otherwise"""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32) if np.array_equal(f32(a), a) else a


def model_rows(model):
    p0, v0, a0, sets = make_inputs(model)
    N = len(sets)
    n = NS[model]
    angular = model in ANGULAR
    now, at = np.zeros((N, 19)), np.zeros((N, 13))
    d_now, branch_now, strict_now = np.zeros((N, 6)), np.zeros(N, np.int8), np.zeros(N, bool)
    tick_cases = np.nonzero((sets != 3) & (np.arange(N) % TICK_EVERY == TICK_PHASE))[0] if angular else np.zeros(0, int)
    M = len(tick_cases)
    x_k, pose_k = np.zeros((TICKS, M, n)), np.zeros((TICKS, M, 7))
    d_k, branch_k, strict_k = np.zeros((TICKS, M, 4)), np.zeros((TICKS, M), np.int8), np.zeros((TICKS, M), bool)
    A = transition_linear(n, 3, mpf(DT)) if model == "angular_rates" else None
    for i in range(N):
        x, d0, d1 = init_state(model, p0[i], v0[i], a0[i])
        o_now, _ = outputs(model, x, mpf(0))
        _, o_at = outputs(model, x, mpf(float(OFFSETS[i % 4])))
        now[i] = fl(o_now[0] + o_now[1] + o_now[2])
        at[i] = fl(o_at[0] + o_at[1])
        if not angular:
            d_now[i] = [9, 9, 3, 9, 9, 1]
            strict_now[i] = True
            continue
        b, tr, gap, d4, c = decisions(x)
        d = [d0, d1, tr, gap, d4, c]
        d_now[i], branch_now[i], strict_now[i] = fl(d), b, is_strict(d)
        if i not in tick_cases:
            continue
        j = int(np.searchsorted(tick_cases, i))
        cmin = c
        for k in range(TICKS):
            x = list(A * matrix(x)) if model == "angular_rates" else ekf_f(x, mpf(DT))
            b, tr, gap, d4, c = decisions(x)
            if model == "angular_rates" or abs(c) < abs(cmin):     # (the linear model's prediction does not divide by it)
                cmin = c
            d = [d0, d1, tr, gap, d4, cmin]
            x_k[k, j] = fl(x)
            pose_k[k, j] = fl(outputs(model, x, mpf(0))[0][0])
            d_k[k, j], branch_k[k, j], strict_k[k, j] = fl(d[2:]), b, is_strict(d)
    gimbal = sets == 3
    group_now = np.where(gimbal, 12, branch_now).astype(np.int8)
    group_at = np.where(gimbal, -1, 4 + branch_now).astype(np.int8)
    group_k = (8 + branch_k).astype(np.int8)
    if angular:
        assert not strict_now[gimbal].any()                  # state pitch = +-pi/2: never strict, by the rule on cos
        assert (np.abs(d_now[:, 0]) >= MARGIN).all()         # nobody sits on the gimbal threshold: across it the STATE differs, not its sign
        assert (np.abs(d_k[:, :, 3]) >= 0.02).all() or model == "angular_rates"       # the EKF's 1 / cos(pitch) stays below 50
        rows = np.concatenate([strict_now, strict_now[~gimbal], strict_k.ravel()])
        share = rows.mean()
        assert share >= 0.90, share
        counts = {}
        for g, name in enumerate(GROUPS[:12]):
            sel = [group_now == g, group_at == g, None][g // 4]
            s = int(strict_now[sel].sum()) if sel is not None else int(strict_k[group_k == g].sum())
            t = int(sel.sum()) if sel is not None else int((group_k == g).sum())
            counts[name] = (s, t)
            assert s >= 24, (model, name, s)
        assert gimbal.sum() >= 24 and (d_now[gimbal, 0] > 0).all() and (d_now[~gimbal, 0] < 0).all()
        past = int((np.abs(x_k[:, :, 4]) > np.pi / 2).any(axis=0).sum())
        if model == "angular_rates":
            assert past >= 24, past
        assert M % 64 and M % 10, M
        print("%-20s %d cases, %d with ticks; strict share of the rows %.3f; state pitch past +-pi/2 within three ticks: %d cases"
              % (model, N, M, share, past))
        print("    strict / all per group: " + "  ".join("%s %d/%d" % (k, *v) for k, v in counts.items()) + "  gimbal 0/%d" % gimbal.sum())
        print("    least margins of the strict rows: gimbal threshold %.3g, atan2 (init) %.3g, |trace| %.3g, diagonal gap %.3g, atan2 (outputs) %.3g, |cos pitch| %.3g"
              % tuple(np.abs(np.concatenate([d_now[strict_now], np.concatenate([d_now[tick_cases][None, :, :2].repeat(TICKS, 0), d_k], 2)[strict_k]])).min(axis=0)))
    else:
        print("%-20s %d cases (control: identity orientation, offsets)" % (model, N))
    out = dict(p0=pack(p0), v0=pack(v0), a0=pack(a0), set=sets,
               now_pos=pack(now[:, 0:3]), now_quat=now[:, 3:7], now_twl=pack(now[:, 7:10]), now_twa=pack(now[:, 10:13]), now_acc=pack(now[:, 13:19]),
               at_pos=pack(at[:, 0:3]), at_quat=at[:, 3:7], at_twl=pack(at[:, 7:10]), at_twa=pack(at[:, 10:13]))
    if angular:
        out.update(d_now=d_now.astype(np.float32), branch_now=branch_now, strict_now=strict_now, group_now=group_now, group_at=group_at,
                   tick_cases=tick_cases.astype(np.int16), xk_rpy=x_k[:, :, 3:6], xk_rest=pack(np.delete(x_k, [3, 4, 5], axis=2)),
                   tick_pos=pack(pose_k[:, :, 0:3]), tick_quat=pose_k[:, :, 3:7],
                   d_k=d_k.astype(np.float32), branch_k=branch_k, strict_k=strict_k, group_k=group_k)
    return {"%s_%s" % (k, model): v for k, v in out.items()}


def main():
    out = dict(dt=np.array(DT), offsets=OFFSETS, groups=np.array(GROUPS))
    for model in MODELS:
        out.update(model_rows(model))
    path = os.path.join(HERE, "attitude_kat.npz")
    np.savez_compressed(path, **out)
    print("attitude_kat.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
