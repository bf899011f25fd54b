"""Growth of a batch leaves every target's bits alone.  Filters are per target, so a target's bits do not depend on its batch
mates -- nor on how often the arrays it lives in have been re-allocated.  Three managers are fed the same calls and the same
streams (conftest.synth_stream):
  A  holds only the 40 early targets and never leaves its first capacity;
  B  holds the same 40 and is grown between ticks by three further init_batch calls to 65, 130 and 700 targets (across a tile
     boundary and through two doublings of the capacity), every array of Batch::reserve re-allocated each time;
  C  holds only the 660 late targets, created by the same calls at the same t0.
Initial covariances are per target.  An update policy (gate, max_rejects = 3) is on, and two by-id ticks with outliers leave some
rejection runs non-zero before the first growth; the measured poses are kept from then on (the by-id policy is not served for a
batch that keeps them, so the later ticks are dense ones).  After every stage the early targets must agree BIT FOR BIT between A
and B, the late ones between B and C, on state, covariance, time, measurement count, rejection run, measured pose and derived
pose.  The f64 case (uniform_velocity, the default layout: shared axes with uniform tiles) goes on with dense ticks after the last
growth, so that the tile arrays re-allocated by the growth are exercised, flagged tiles included."""
import numpy as np
import pytest

import gate_ref
import oracle
from conftest import model_path, synth_stream

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
te = pytest.importorskip("target_estimation_amd")

DT = 0.004
SIZES = (40, 65, 130, 700)   # B's size after its creation and after each growth
IDS = np.arange(SIZES[-1], dtype=np.uint32) * 5 + 2
EARLY, LATE = IDS[:SIZES[0]], IDS[SIZES[0]:]
MAX_REJECTS = 3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _everything(mgr, ids):
    """all that is compared, of the ids given, in their order"""
    x, P = mgr.get_state_batch(ids)
    pose, twist, acc, found = mgr.get_est_batch(ids)
    assert found.all()
    measured = [mgr.getMeasuredPose(int(i)) for i in ids] if mgr.kept else []
    return dict(x=x, P=P,
                t=np.array([mgr.getTime(int(i)) for i in ids]),
                nm=np.array([mgr.getNumberMeasurements(int(i)) for i in ids]),
                run=np.array([mgr.getRejectionRun(int(i)) for i in ids]),
                measured_ok=np.array([ok for ok, _ in measured]),
                measured=np.array([row for _, row in measured]),
                pose=pose, twist=twist, acc=acc)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (what, k)


def _soa(rows, dtype):
    tdt = torch.float64 if dtype == "f64" else torch.float32
    return torch.from_numpy(np.ascontiguousarray(rows.T)).to("cuda").to(tdt).contiguous()


@pytest.mark.parametrize("name,dtype", [("uniform_velocity", "f64"), ("angular_velocities", "f32")])
def test_growth_leaves_every_target_alone(name, dtype):
    model = oracle.load_model_yaml(model_path(name))
    n_ticks = 10
    p0, meas = synth_stream(name, SIZES[-1], n_ticks, seed=23, dt=DT)
    gamma = gate_ref.CHI2_99[gate_ref.m_of(name)]
    # per-target initial covariances: a scalar multiple of the model's each (the shared-axes form stays); the early targets and a
    # few late ones differ from their neighbours, most late targets agree (so that whole tiles of them can become uniform)
    rng = np.random.default_rng(5)
    scale = np.ones(SIZES[-1])
    scale[:SIZES[0]] = rng.choice([1.0, 1.5, 2.0], SIZES[0])
    scale[SIZES[0]:SIZES[2]] = rng.choice([1.0, 1.25], SIZES[2] - SIZES[0])
    scale[[300, 301, 699]] = 3.0
    P0 = np.asarray(model["P"], dtype=np.float64)[None, :, :] * scale[:, None, None]

    def create(mgr, lo, hi, t0):
        assert mgr.init_batch(IDS[lo:hi], DT, t0, p0[lo:hi], type=model["model"], Q=model["Q"], R=model["R"], P0=P0[lo:hi]) == hi - lo

    def manager():
        mgr = te.TargetManager(model_path(name), dtype=dtype)
        mgr.set_update_gate(gamma, MAX_REJECTS)
        mgr.kept = False
        return mgr

    def keep(mgr):
        mgr.set_keep_measurement(True)
        mgr.kept = True

    def dense_tick(mgr, s, lo, hi):
        (b,) = mgr.batches()
        assert b.size == hi - lo
        b.step(DT, _soa(meas[s, lo:hi], dtype))

    A, B, C = manager(), manager(), manager()
    keep(C)   # (C serves no by-id tick)
    ticks = 0
    try:
        for mgr in (A, B):
            create(mgr, 0, SIZES[0], 0.0)
        if dtype == "f64":
            assert B.batches()[0].shared_axes and B.batches()[0].layout == "axis_separable_packed"
        # two by-id ticks under the policy; a third of the early targets get outliers on both: rejection runs of 2 before any growth
        out = meas[:2, :SIZES[0]].copy()
        out[:, ::3, :3] += 50.0
        for s in range(2):
            for mgr in (A, B):
                done, nis, ev = mgr.update_batch(EARLY, DT, out[s], None, gated=True)
                assert done == SIZES[0] and (nis[::3] > gamma).all()
            ticks += 1
        for mgr in (A, B):
            keep(mgr)
        a = _everything(A, EARLY)
        assert (a["run"][::3] == 2).all() and a["run"].max() == 2
        _same(a, _everything(B, EARLY), "before the first growth, early")
        # the three growths, two dense ticks behind each of the first two
        for g in range(1, len(SIZES)):
            lo, hi = SIZES[g - 1], SIZES[g]
            t0 = ticks * DT
            create(B, lo, hi, t0)
            create(C, lo, hi, t0)
            assert B.size() == hi and C.size() == hi - SIZES[0]
            what = "after growth %d (%d targets)" % (g, hi)
            _same(_everything(A, EARLY), _everything(B, EARLY), what + ", early")
            _same(_everything(B, IDS[SIZES[0]:hi]), _everything(C, IDS[SIZES[0]:hi]), what + ", late")
            if g == len(SIZES) - 1:
                break
            for _ in range(2):
                dense_tick(A, ticks, 0, SIZES[0])
                dense_tick(B, ticks, 0, hi)
                dense_tick(C, ticks, SIZES[0], hi)
                ticks += 1
            what = "two ticks behind growth %d" % g
            _same(_everything(A, EARLY), _everything(B, EARLY), what + ", early")
            _same(_everything(B, IDS[SIZES[0]:hi]), _everything(C, IDS[SIZES[0]:hi]), what + ", late")
        if dtype == "f64":
            # dense ticks over the tile arrays the last growth allocated: two, and two more, by which whole tiles of agreeing late
            # targets are flagged uniform (in B and in C they are different tiles)
            for rnd in range(2):
                for _ in range(2):
                    dense_tick(A, ticks, 0, SIZES[0])
                    dense_tick(B, ticks, 0, SIZES[-1])
                    dense_tick(C, ticks, SIZES[0], SIZES[-1])
                    ticks += 1
                if rnd == 1:
                    assert B.batches()[0].uniform_tiles > 0 and C.batches()[0].uniform_tiles > 0
                what = "%d dense ticks behind the last growth" % (2 * rnd + 2)
                _same(_everything(A, EARLY), _everything(B, EARLY), what + ", early")
                _same(_everything(B, LATE), _everything(C, LATE), what + ", late")
        assert ticks <= n_ticks
    finally:
        for mgr in (A, B, C):
            mgr.close()
