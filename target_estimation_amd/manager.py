"""Python front-end over the C ABI (ctypes).  Mirrors the reference's TargetManager method names
(include/target_estimation/target_manager.hpp:66-203); every numeric call goes through
libtarget_estimation_amd.so and runs on the GPU.  torch is used only for device buffers/streams.
"""
import ctypes as C

import numpy as np

from . import capi

ANGULAR_RATES, ANGULAR_VELOCITIES, UNIFORM_ACCELERATION, UNIFORM_VELOCITY = 0, 1, 2, 3
TARGET_ASSOC_GRID_MAX_DETECTIONS = 1048576   # the most detections of a frame in the grid form of associate (target_batch_c.h)
MODEL_TYPES = {"angular_rates": 0, "angular_velocities": 1, "uniform_acceleration": 2, "uniform_velocity": 3}
MODEL_DIMS = {0: (18, 6), 1: (12, 6), 2: (9, 3), 3: (6, 3)}
DTYPES = {"f64": 0, "f32": 1}
SYMMETRIC_PACKED = 100   # add to lanes_per_target=1: upper triangle of P only in HBM
AXIS_SEPARABLE = 200     # add to lanes_per_target=1: only the per-axis blocks of P (exact for decoupled Q, R, P0)


def _dp(a):
    return None if a is None else a.ctypes.data_as(capi.c_double_p)


def _d(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ids(ids):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    return ids, ids.ctypes.data_as(capi.c_uint_p)


def _model_type(type):
    return MODEL_TYPES[type] if isinstance(type, str) else int(type)


def _check(rc, what):
    if rc is None or rc < 0:
        raise RuntimeError("%s failed: %s" % (what, capi.last_error()))
    return rc


def _pose_stream(poses, size, n_ticks):
    """A float64 CUDA tensor [blocks, 7, ld] (or [7, ld]: one block every tick overwrites) -> capi.PoseStream.  ld and
    tick_stride come from its strides; fewer blocks than ticks make it a ring (tick s writes block s % blocks)."""
    import torch
    assert poses.is_cuda and poses.dtype == torch.float64, "poses: a float64 CUDA tensor"
    if poses.dim() == 2:
        poses = poses.unsqueeze(0)
    assert poses.dim() == 3 and poses.shape[1] == 7 and poses.stride(2) == 1, "poses: [ticks_or_ring, 7, ld] with unit stride along the slots"
    if poses.shape[2] < size:
        raise RuntimeError("pose stream: %d columns for a batch of %d targets" % (poses.shape[2], size))
    ps = capi.PoseStream()
    ps.pose_dev, ps.ld = poses.data_ptr(), poses.stride(1)
    ps.tick_stride = poses.stride(0) if poses.shape[0] > 1 else 0
    ps.ring_ticks = poses.shape[0] if poses.shape[0] < n_ticks else 0
    return ps


def _innov_stream(innov, size, m, n_ticks):
    """(nis, nu): float64 CUDA tensors [blocks, ld] (or [ld]) and [blocks, m, ld] (or [m, ld]), nu may be None (NIS only) ->
    capi.InnovStream.  One block: every tick overwrites it; fewer blocks than ticks make a ring, as for poses."""
    import torch
    nis, nu = innov
    assert nis.is_cuda and nis.dtype == torch.float64, "innov: nis is a float64 CUDA tensor"
    if nis.dim() == 1:
        nis = nis.unsqueeze(0)
    assert nis.dim() == 2 and nis.stride(1) == 1, "innov: nis is [ticks_or_ring, ld] with unit stride along the slots"
    if nis.shape[1] < size:
        raise RuntimeError("innovation stream: %d columns for a batch of %d targets" % (nis.shape[1], size))
    s = capi.InnovStream()
    s.nis_dev, s.ld = nis.data_ptr(), nis.shape[1]
    s.nis_tick_stride = nis.stride(0) if nis.shape[0] > 1 else 0
    s.ring_ticks = nis.shape[0] if nis.shape[0] < n_ticks else 0
    if nu is not None:
        assert nu.is_cuda and nu.dtype == torch.float64, "innov: nu is a float64 CUDA tensor"
        if nu.dim() == 2:
            nu = nu.unsqueeze(0)
        assert nu.dim() == 3 and nu.shape[0] == nis.shape[0] and nu.shape[1] == m and nu.stride(2) == 1 and nu.stride(1) == s.ld, \
            "innov: nu is [blocks, m, ld] with as many blocks and the same ld as nis"
        s.innov_dev = nu.data_ptr()
        s.innov_tick_stride = nu.stride(0) if nu.shape[0] > 1 else 0
    return s


def _dt_schedule(dt, n_ticks):
    """dt of a multi-tick call: a number -> None (the scalar calls, exactly as ever); a sequence or array -> its float64 copy, one
    entry per tick of the call (the ..._dt calls).  A wrong length raises ValueError before any library call."""
    if np.ndim(dt) == 0:
        return None
    sched = np.ascontiguousarray(dt, dtype=np.float64)
    if sched.ndim != 1 or sched.shape[0] != int(n_ticks):
        raise ValueError("dt: a time-step schedule has one entry per tick: expected %d, got shape %s" % (int(n_ticks), sched.shape))
    return sched


def _reacquire(policy, size, n_ticks):
    """(K, events_or_None) -> capi.Reacquire.  events: uint8 CUDA tensor [blocks, ld] (or [ld]): one block, every tick overwrites
    it; fewer blocks than ticks make a ring, as for the innovation stream.  None: no policy (max_rejects = -1)."""
    import torch
    r = capi.Reacquire()
    if policy is None:
        r.max_rejects = -1
        return r
    k, ev = policy
    r.max_rejects = int(k)
    if ev is not None:
        assert ev.is_cuda and ev.dtype == torch.uint8, "reacquire: events is a uint8 CUDA tensor"
        if ev.dim() == 1:
            ev = ev.unsqueeze(0)
        assert ev.dim() == 2 and ev.stride(1) == 1, "reacquire: events is [ticks_or_ring, ld] with unit stride along the slots"
        r.event_dev, r.ld = ev.data_ptr(), ev.shape[1]
        r.tick_stride = ev.stride(0) if ev.shape[0] > 1 else 0
        r.ring_ticks = ev.shape[0] if ev.shape[0] < n_ticks else 0
    return r


class Batch:
    """All targets of one (model, Q, R) of a manager: the device-resident dense path."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle

    size = property(lambda s: s._lib.target_batch_size(s._h))
    type = property(lambda s: s._lib.target_batch_type(s._h))
    dtype = property(lambda s: "f64" if s._lib.target_batch_dtype(s._h) == 0 else "f32")
    state_dim = property(lambda s: s._lib.target_batch_state_dim(s._h))
    meas_dim = property(lambda s: s._lib.target_batch_meas_dim(s._h))
    lanes_per_target = property(lambda s: s._lib.target_batch_lanes_per_target(s._h))
    symmetric_packed = property(lambda s: bool(s._lib.target_batch_is_symmetric_packed(s._h)))
    layout = property(lambda s: ("full", "symmetric_packed", "axis_separable", "axis_separable_packed")[s._lib.target_batch_layout(s._h)])
    # the shared-axes storage form of axis_separable_packed (target_batch_shared_axes): one covariance block per kind of axis
    shared_axes = property(lambda s: s._lib.target_batch_shared_axes(s._h))
    # tiles of the batch whose 64 targets share one copy of their linear-chain covariance words now (target_batch_uniform_tiles;
    # reads the flags back: synchronises)
    uniform_tiles = property(lambda s: s._lib.target_batch_uniform_tiles(s._h))
    record_words = property(lambda s: s._lib.target_batch_record_words(s._h))
    num_classes = property(lambda s: s._lib.target_batch_num_classes(s._h))
    algorithmic_bytes = property(lambda s: s._lib.target_batch_algorithmic_bytes(s._h))
    resident_bytes_per_target = property(lambda s: s._lib.target_batch_resident_bytes_per_target(s._h))

    def slot_ids(self):
        n = self.size
        out = np.empty(n, dtype=np.uint32)
        self._lib.target_batch_slot_ids(self._h, out.ctypes.data_as(capi.c_uint_p), n)
        return out

    def torch_dtype(self):
        import torch
        return torch.float64 if self.dtype == "f64" else torch.float32

    def step(self, dt, meas=None, has_meas=None):
        """One tick over every target.  meas: CUDA tensor [7, ld] (SoA, batch precision) or None
        (predict only); has_meas: CUDA uint8 tensor [size] or None.  Asynchronous."""
        mp, ld, hp = None, 0, None
        if meas is not None:
            assert meas.is_cuda and meas.dim() == 2 and meas.shape[0] == 7 and (meas.shape[1] == 1 or meas.stride(1) == 1)
            assert meas.dtype == self.torch_dtype(), (meas.dtype, self.dtype)
            assert meas.shape[1] >= self.size
            mp, ld = meas.data_ptr(), meas.stride(0)
        if has_meas is not None:
            assert has_meas.is_cuda and has_meas.numel() >= self.size and has_meas.element_size() == 1
            hp = has_meas.data_ptr()
        _check(self._lib.target_batch_step(self._h, float(dt), mp, ld, hp), "target_batch_step")

    def step_host(self, dt, meas_soa, has_meas=None):
        """One tick from HOST measurements: meas_soa = CPU tensor or ndarray [rows >= 3 or 7, ld] in the batch
        precision (SoA; rows >= 7 for the angular models; pinned memory gives asynchronous DMA), has_meas = CPU uint8 [size] or None."""
        import torch
        t = meas_soa if isinstance(meas_soa, torch.Tensor) else torch.from_numpy(meas_soa)
        assert not t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype == self.torch_dtype() and t.shape[1] >= self.size
        need = 7 if self.type in (ANGULAR_RATES, ANGULAR_VELOCITIES) else 3   # rows the model reads (and the copy moves)
        assert t.shape[0] >= need, "this model reads %d measurement rows, got %d" % (need, t.shape[0])
        hp = None
        if has_meas is not None:
            h = has_meas if isinstance(has_meas, torch.Tensor) else torch.from_numpy(has_meas)
            assert not h.is_cuda and h.element_size() == 1 and h.numel() >= self.size
            hp = h.data_ptr()
        _check(self._lib.target_batch_step_host(self._h, float(dt), t.data_ptr(), t.stride(0), hp), "target_batch_step_host")

    def rejection_runs(self):
        """The run of consecutive gate rejections of every slot (uint8, slot order), as the calls with reacquire= keep it
        (target_batch_rejection_runs); synchronises."""
        out = np.zeros(max(self.size, 1), dtype=np.uint8)
        _check(self._lib.target_batch_rejection_runs(self._h, out.ctypes.data), "target_batch_rejection_runs")
        return out[:self.size]

    def track_counts(self):
        """(miss, hits) of every slot (uint8, slot order): the run of consecutive lifecycle calls without a match and the calls with
        one since creation, as TargetManager.lifecycle keeps them (target_batch_track_counts); synchronises."""
        n = self.size
        miss, hits = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
        _check(self._lib.target_batch_track_counts(self._h, miss.ctypes.data_as(capi.c_ubyte_p), hits.ctypes.data_as(capi.c_ubyte_p)),
               "target_batch_track_counts")
        return miss[:n], hits[:n]

    def step_sequence(self, dt, meas, has_meas=None, use_graph=False, n_ticks=None, poses=None, innov=None, gate=None, reacquire=None):
        """meas: CUDA tensor [ticks, 7, ld]: one launch per tick, all enqueued by one C call.  n_ticks > ticks
        treats meas (and has_meas) as a ring: tick s reads entry s % ticks.  poses: float64 CUDA tensor
        [ticks_or_ring, 7, ld] (or [7, ld]) that receives every target's pose after every tick (column = slot;
        target_batch_step_sequence_poses); fewer blocks than ticks make it a ring.  innov = (nis, nu_or_None): float64 CUDA
        tensors [ticks_or_ring, ld] and [ticks_or_ring, m, ld] that receive every tick's NIS and innovations
        (target_batch_step_sequence_innov; -1 and zeros for a target without a measurement on the tick).  gate = nis_max: the
        NIS validation gate inside the ticks (target_batch_step_sequence_gated): a measurement with NIS > nis_max, or a NaN one,
        is not folded in -- the target is stepped as without a measurement -- and the stream still reports its NIS and nu, so the
        decision is 0 <= nis <= nis_max.  Needs innov; 0 or None: no gate.  reacquire = (K, events_or_None): re-acquisition
        inside the gated ticks (target_batch_step_sequence_reacquire): every slot's run of consecutive rejections is kept on the
        device (rejection_runs()), and on its K-th consecutive rejection a target is re-initialised from that tick's
        measurement with its own initial covariance (K = 0: count only); events: uint8 CUDA tensor [ticks_or_ring, ld] (or
        [ld]) that receives every tick's event bytes (0, the run c', or 0x80 | c' for a re-initialisation).  Needs gate.
        dt: a number, or a sequence / array with one time step per tick of the call (target_batch_step_sequence_dt): tick s
        runs with dt[s], per slot the results of step(dt[s], ...) tick after tick, bit for bit, the target's time included.  A
        recorded graph (use_graph) is reused by a call with the same schedule, value for value."""
        sched = _dt_schedule(dt, meas.shape[0] if n_ticks is None else n_ticks)
        assert meas.is_cuda and meas.dim() == 3 and meas.shape[1] == 7 and (meas.shape[2] == 1 or meas.stride(2) == 1)
        assert meas.dtype == self.torch_dtype() and meas.shape[2] >= self.size
        hp, hs = None, 0
        if has_meas is not None:
            assert has_meas.is_cuda and has_meas.dim() == 2 and has_meas.element_size() == 1
            hp, hs = has_meas.data_ptr(), has_meas.stride(0)
        if sched is not None:
            ticks = sched.shape[0]
            ps = _pose_stream(poses, self.size, ticks) if poses is not None else None
            ins = _innov_stream(innov, self.size, self.meas_dim, ticks) if innov is not None else None
            rq = _reacquire(reacquire, self.size, ticks) if reacquire is not None else None
            _check(self._lib.target_batch_step_sequence_dt(
                self._h, ticks, sched.ctypes.data_as(capi.c_double_p), meas.data_ptr(), meas.stride(0), meas.stride(1), hp, hs,
                meas.shape[0] if ticks != meas.shape[0] else 0, None if ps is None else C.byref(ps), None if ins is None else C.byref(ins),
                0.0 if gate is None else float(gate), None if rq is None else C.byref(rq), int(use_graph)), "target_batch_step_sequence_dt")
            return
        if innov is not None or gate is not None or reacquire is not None:   # (a gate without a stream, a policy without a gate: the library's to refuse)
            ticks = meas.shape[0] if n_ticks is None else int(n_ticks)
            ps = _pose_stream(poses, self.size, ticks) if poses is not None else None
            ins = _innov_stream(innov, self.size, self.meas_dim, ticks) if innov is not None else None
            args = (self._h, ticks, float(dt), meas.data_ptr(), meas.stride(0), meas.stride(1), hp, hs,
                    meas.shape[0] if ticks != meas.shape[0] else 0, None if ps is None else C.byref(ps), None if ins is None else C.byref(ins))
            if reacquire is not None:
                rq = _reacquire(reacquire, self.size, ticks)
                _check(self._lib.target_batch_step_sequence_reacquire(*args, 0.0 if gate is None else float(gate), C.byref(rq), int(use_graph)),
                       "target_batch_step_sequence_reacquire")
            elif gate is not None:
                _check(self._lib.target_batch_step_sequence_gated(*args, float(gate), int(use_graph)), "target_batch_step_sequence_gated")
            else:
                _check(self._lib.target_batch_step_sequence_innov(*args, int(use_graph)), "target_batch_step_sequence_innov")
            return
        if poses is not None:
            ticks = meas.shape[0] if n_ticks is None else int(n_ticks)
            ps = _pose_stream(poses, self.size, ticks)
            _check(self._lib.target_batch_step_sequence_poses(self._h, ticks, float(dt), meas.data_ptr(), meas.stride(0), meas.stride(1),
                                                               hp, hs, meas.shape[0] if ticks != meas.shape[0] else 0, C.byref(ps),
                                                               int(use_graph)), "target_batch_step_sequence_poses")
            return
        if n_ticks is None or n_ticks == meas.shape[0]:
            _check(self._lib.target_batch_step_sequence(self._h, meas.shape[0], float(dt), meas.data_ptr(), meas.stride(0),
                                                         meas.stride(1), hp, hs, int(use_graph)),
                   "target_batch_step_sequence")
        else:
            _check(self._lib.target_batch_step_sequence_ring(self._h, int(n_ticks), float(dt), meas.data_ptr(), meas.stride(0),
                                                              meas.stride(1), hp, hs, meas.shape[0], int(use_graph)),
                   "target_batch_step_sequence_ring")

    def step_fused(self, dt, meas, has_meas=None, poses=None, innov=None, gate=None, reacquire=None):
        """meas: CUDA tensor [ticks, 7, ld]: all ticks in ONE launch (state stays in registers).  poses: as for
        step_sequence (target_batch_step_fused_poses).  innov, gate, reacquire: the keywords of step_sequence with their
        meanings there, served inside the fused call (target_batch_step_fused_gated): per slot and tick the results of
        step_sequence(dt, meas, has_meas, poses=, innov=, gate=, reacquire=) bit for bit -- one launch for the whole call where
        fused_gate_served is 1 and no poses are asked for, tick by tick inside the call otherwise.
        dt: a number, or a sequence / array with one time step per tick (target_batch_step_fused_dt): tick s runs with dt[s], the
        results of step(dt[s], ...) tick after tick, bit for bit -- one launch where fused_dt_served(gated) is 1 and no poses are
        asked for."""
        sched = _dt_schedule(dt, meas.shape[0])
        assert meas.is_cuda and meas.dim() == 3 and meas.shape[1] == 7 and (meas.shape[2] == 1 or meas.stride(2) == 1)
        assert meas.dtype == self.torch_dtype() and meas.shape[2] >= self.size
        hp, hs = None, 0
        if has_meas is not None:
            assert has_meas.is_cuda and has_meas.dim() == 2 and has_meas.element_size() == 1
            hp, hs = has_meas.data_ptr(), has_meas.stride(0)
        if sched is not None:
            ticks = sched.shape[0]
            ps = _pose_stream(poses, self.size, ticks) if poses is not None else None
            ins = _innov_stream(innov, self.size, self.meas_dim, ticks) if innov is not None else None
            rq = _reacquire(reacquire, self.size, ticks) if reacquire is not None else None
            _check(self._lib.target_batch_step_fused_dt(
                self._h, ticks, sched.ctypes.data_as(capi.c_double_p), meas.data_ptr(), meas.stride(0), meas.stride(1), hp, hs,
                None if ps is None else C.byref(ps), None if ins is None else C.byref(ins),
                0.0 if gate is None else float(gate), None if rq is None else C.byref(rq)), "target_batch_step_fused_dt")
            return
        if innov is not None or gate is not None or reacquire is not None:   # (a gate without a stream, a policy without a gate: the library's to refuse)
            ticks = meas.shape[0]
            ps = _pose_stream(poses, self.size, ticks) if poses is not None else None
            ins = _innov_stream(innov, self.size, self.meas_dim, ticks) if innov is not None else None
            rq = _reacquire(reacquire, self.size, ticks) if reacquire is not None else None
            _check(self._lib.target_batch_step_fused_gated(self._h, ticks, float(dt), meas.data_ptr(), meas.stride(0), meas.stride(1), hp, hs,
                                                            None if ps is None else C.byref(ps), None if ins is None else C.byref(ins),
                                                            0.0 if gate is None else float(gate), None if rq is None else C.byref(rq)),
                   "target_batch_step_fused_gated")
            return
        if poses is not None:
            ps = _pose_stream(poses, self.size, meas.shape[0])
            _check(self._lib.target_batch_step_fused_poses(self._h, meas.shape[0], float(dt), meas.data_ptr(), meas.stride(0),
                                                            meas.stride(1), hp, hs, C.byref(ps)), "target_batch_step_fused_poses")
            return
        _check(self._lib.target_batch_step_fused(self._h, meas.shape[0], float(dt), meas.data_ptr(), meas.stride(0),
                                                  meas.stride(1), hp, hs), "target_batch_step_fused")

    # 1: a fused call with innov= / gate= / reacquire= (and without poses=) is one launch; 0: served tick by tick inside the call
    fused_gate_served = property(lambda s: s._lib.target_batch_step_fused_gate_served(s._h))

    def fused_dt_served(self, gated=False):
        """1: a fused call with a time-step schedule (and without poses=) is one launch -- gated: a call with innov= / gate= /
        reacquire= --; 0: served tick by tick inside the call (target_batch_step_fused_dt_served)."""
        return _check(self._lib.target_batch_step_fused_dt_served(self._h, 1 if gated else 0), "target_batch_step_fused_dt_served")

    # recordings made so far by step_sequence(..., use_graph=True) on this batch (target_batch_graph_recordings)
    graph_recordings = property(lambda s: s._lib.target_batch_graph_recordings(s._h))

    # ---- resident ("live") mode: one launch serves tick after tick as the host posts them (target_batch_c.h)
    def live_start(self, dt, meas_ring, has_ring=None, first_entry=0, max_ticks=1 << 30, idle_limit_s=10.0):
        """meas_ring: CUDA tensor [ring_ticks, 7, ld] in the batch precision; has_ring: CUDA uint8 [ring_ticks, >= size] or None."""
        assert meas_ring.is_cuda and meas_ring.dim() == 3 and meas_ring.shape[1] == 7 and meas_ring.stride(2) == 1
        assert meas_ring.dtype == self.torch_dtype() and meas_ring.shape[2] >= self.size
        hp, hs = None, 0
        if has_ring is not None:
            assert has_ring.is_cuda and has_ring.dim() == 2 and has_ring.element_size() == 1 and has_ring.shape[0] == meas_ring.shape[0]
            hp, hs = has_ring.data_ptr(), has_ring.stride(0)
        _check(self._lib.target_batch_live_start(self._h, float(dt), meas_ring.data_ptr(), meas_ring.stride(0), meas_ring.stride(1), hp, hs,
                                                 meas_ring.shape[0], int(first_entry), int(max_ticks), float(idle_limit_s)), "target_batch_live_start")

    def live_set_pose_output(self, pose_soa):
        """pose_soa: CUDA double tensor [7, ld >= size] (or None): sessions started afterwards write every tick's poses there."""
        if pose_soa is None:
            _check(self._lib.target_batch_live_set_pose_output(self._h, None, 0), "target_batch_live_set_pose_output")
            return
        import torch
        assert pose_soa.is_cuda and pose_soa.dtype == torch.float64 and pose_soa.dim() == 2 and pose_soa.shape[0] == 7 and pose_soa.stride(1) == 1
        _check(self._lib.target_batch_live_set_pose_output(self._h, pose_soa.data_ptr(), pose_soa.stride(0)), "target_batch_live_set_pose_output")

    def live_set_gate(self, nis_max, nis_rows, reacquire=None):
        """The NIS gate and, with reacquire=, the re-acquisition policy INSIDE the sessions started afterwards
        (target_batch_live_set_gate), in the conventions of step_sequence(..., innov=, gate=, reacquire=).  nis_max: the gate (0 or
        None: off; inf: gated, everything finite accepted).  nis_rows: float64 CUDA tensor [rows, ld] (or [ld]) that receives
        tick k's NIS in row k % rows (one row: every tick overwrites it); None with nis_max off.  reacquire = (K, events_or_None),
        events a uint8 CUDA tensor [rows, ld] (or [ld]) with its own ring of rows.  A consumer may copy row k % rows on another
        stream once live_done() has reached k + 1.  live_capacity then reports the gated kernel's capacity."""
        if not nis_max and nis_rows is None and reacquire is None:
            _check(self._lib.target_batch_live_set_gate(self._h, 0.0, None, None), "target_batch_live_set_gate")
            return
        ins = _innov_stream((nis_rows, None), self.size, self.meas_dim, 1 << 62) if nis_rows is not None else None
        rq = _reacquire(reacquire, self.size, 1 << 62) if reacquire is not None else None
        _check(self._lib.target_batch_live_set_gate(self._h, 0.0 if nis_max is None else float(nis_max), None if ins is None else C.byref(ins),
                                                    None if rq is None else C.byref(rq)), "target_batch_live_set_gate")

    live_gate_served = property(lambda s: s._lib.target_batch_live_gate_served(s._h))

    def live_post(self, n_ticks=1):
        _check(self._lib.target_batch_live_post(self._h, int(n_ticks)), "target_batch_live_post")

    def live_post_each(self, n_ticks):
        _check(self._lib.target_batch_live_post_each(self._h, int(n_ticks)), "target_batch_live_post_each")

    def live_done(self):
        return self._lib.target_batch_live_done(self._h)

    def live_wait(self, tick, timeout_s=5.0):
        rc = _check(self._lib.target_batch_live_wait(self._h, int(tick), float(timeout_s)), "target_batch_live_wait")
        return rc == 0

    def live_stop(self):
        return _check(self._lib.target_batch_live_stop(self._h), "target_batch_live_stop")

    live_capacity = property(lambda s: s._lib.target_batch_live_capacity(s._h))

    def live_running(self):
        """True while the session's resident kernel is there (it leaves after live_stop, or by itself after the idle limit)."""
        return self._lib.target_batch_live_running(self._h) == 1

    def get_est(self, pose=True, twist=True, acc=True, t1=None):
        """Derived outputs of every slot as CUDA double tensors ([size,7], [size,6], [size,6])."""
        import torch
        n = self.size
        mk = lambda w, on: torch.empty((n, w), dtype=torch.float64, device="cuda") if on else None  # noqa: E731
        p, t, a = mk(7, pose), mk(6, twist), mk(6, acc)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        _check(self._lib.target_batch_get_est_dev(self._h, ptr(p), ptr(t), ptr(a), 0 if t1 is None else 1,
                                                   0.0 if t1 is None else float(t1)), "target_batch_get_est_dev")
        return p, t, a

    def intersect_sphere(self, origin, radius, t1=None, want_pose=True):
        """Sphere-intersection query for every slot: (delta [size], pose [size,7] or None) as CUDA double
        tensors; t1=None queries each target at its own current time."""
        import torch
        n = self.size
        delta = torch.empty(n, dtype=torch.float64, device="cuda")
        pose = torch.empty((n, 7), dtype=torch.float64, device="cuda") if want_pose else None
        origin = _d(origin, (3,))
        _check(self._lib.target_batch_intersect_sphere_dev(
            self._h, float("nan") if t1 is None else float(t1), _dp(origin), float(radius), delta.data_ptr(),
            None if pose is None else pose.data_ptr()), "target_batch_intersect_sphere_dev")
        return delta, pose

    def intersect_sphere_converged(self, origin, radius, pos_th, ang_th, t1=None, filters_length=250):
        import torch
        n = self.size
        delta = torch.empty(n, dtype=torch.float64, device="cuda")
        pose = torch.empty((n, 7), dtype=torch.float64, device="cuda")
        conv = torch.empty(n, dtype=torch.uint8, device="cuda")
        origin = _d(origin, (3,))
        _check(self._lib.target_batch_intersect_sphere_converged_dev(
            self._h, float("nan") if t1 is None else float(t1), float(pos_th), float(ang_th), _dp(origin), float(radius),
            int(filters_length), delta.data_ptr(), pose.data_ptr(), conv.data_ptr()), "target_batch_intersect_sphere_converged_dev")
        return conv, pose, delta

    def gate_update(self, delta, pose, pos_th, ang_th, filters_length=250, want_variance=False):
        """The convergence gate alone on query results already on the device (delta [size], pose [size,7], CUDA doubles):
        returns converged [size] uint8, filtered errors [size,2] and, on request, the filters' variances [size,2]."""
        import torch
        n = self.size
        assert delta.is_cuda and pose.is_cuda and delta.dtype == torch.float64 and pose.dtype == torch.float64
        assert delta.numel() >= n and pose.is_contiguous() and pose.shape[0] >= n and pose.shape[1] == 7
        conv = torch.empty(n, dtype=torch.uint8, device="cuda")
        filt = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        var = torch.empty((n, 2), dtype=torch.float64, device="cuda") if want_variance else None
        _check(self._lib.target_batch_gate_update_dev(self._h, delta.data_ptr(), pose.data_ptr(), float(pos_th), float(ang_th),
                                                       int(filters_length), conv.data_ptr(), filt.data_ptr(),
                                                       None if var is None else var.data_ptr()), "target_batch_gate_update_dev")
        return conv, filt, var

    def select_soonest(self, delta, pose=None, ok=None, k=8, window=(0.0, float("inf")), device=False, out=None):
        """The k soonest sphere crossings among this batch's query results on the device (target_batch_select_soonest[_dev]):
        delta [size] and pose [size, 7] (or None: no gather) CUDA doubles, ok [size] a CUDA uint8 / bool mask or None.
        Candidates are the slots with ok != 0 and window[0] <= delta <= window[1], ordered by (delta, slot).
        device=False -> (count, ids [k] uint32, slots [k] int32, delta [k], pose [k, 7] or None) as NumPy arrays, after one small
        copy and a synchronisation; rows count .. k-1 are id 0xffffffff, slot -1, delta -1, pose [0 0 0 0 0 0 1].
        device=True -> (count [1] int32, slots [k] int32, delta [k], pose [k, 7] or None) CUDA tensors, enqueued on the batch's
        stream without a host wait.  Slots (and so a device result) are valid until the next erase or init of the batch.
        out: the output arrays to use, in the order returned (without count for device=False; None entries are passed as NULL)."""
        import torch
        k = int(k)
        ptr = lambda t: None if t is None else t.data_ptr()
        if device:
            if out is None:
                kk = max(k, 1)
                out = (torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(kk, dtype=torch.int32, device="cuda"),
                       torch.empty(kk, dtype=torch.float64, device="cuda"),
                       None if pose is None else torch.empty((kk, 7), dtype=torch.float64, device="cuda"))
            cnt, so, do, po = out
            _check(self._lib.target_batch_select_soonest_dev(self._h, ptr(delta), ptr(pose), ptr(ok), float(window[0]), float(window[1]), k,
                                                             ptr(so), ptr(do), ptr(po), ptr(cnt)), "target_batch_select_soonest_dev")
            return cnt, so, do, po
        if out is None:
            kk = max(k, 1)
            out = (np.empty(kk, dtype=np.uint32), np.empty(kk, dtype=np.int32), np.empty(kk), None if pose is None else np.empty((kk, 7)))
        ids, so, do, po = out
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
        count = _check(self._lib.target_batch_select_soonest(self._h, ptr(delta), ptr(pose), ptr(ok), float(window[0]), float(window[1]), k,
                                                             None if ids is None else ids.ctypes.data_as(capi.c_uint_p), ip(so), _dp(do), _dp(po)),
                       "target_batch_select_soonest")
        return count, ids, so, do, po

    def crossing_cov(self, delta, slots=None, origin=None, radius=0.0, t1=float("nan"), sigma_r_max=float("inf"), sigma_t_max=float("inf"),
                     want_ok=None, out=None):
        """Position covariance and time spread at the sphere crossings (target_batch_crossing_cov_dev), on the batch's stream, no
        host wait.  delta: CUDA doubles, [size] of a query (slots=None: row i is slot i) or [n] alongside slots, a CUDA int32
        list of n <= 8192 slots (-1: none) -- the slots / delta a select_soonest(device=True) returned.  t1: the query's time (NaN:
        each target's own).  Returns (cov [n, 6] = Sigma's upper triangle xx xy xz yy yz zz, sigma [n, 2] = (sigma_r, sigma_t) or
        None without origin, ok [n] uint8 = sigma_r <= sigma_r_max and sigma_t <= sigma_t_max or None) as CUDA tensors; ok is made
        when origin is given unless want_ok=False.  Rows whose delta is negative or NaN (or whose slot is -1) are cov 0, sigma
        (-1, -1), ok 0.  out: (cov, sigma, ok) to use; None entries are passed as NULL."""
        import torch
        n = int(delta.shape[0])
        origin = _d(origin, (3,))
        ptr = lambda t: None if t is None else t.data_ptr()
        if out is None:
            with_ok = (origin is not None) if want_ok is None else bool(want_ok)
            out = (torch.empty((n, 6), dtype=torch.float64, device="cuda"),
                   None if origin is None else torch.empty((n, 2), dtype=torch.float64, device="cuda"),
                   torch.empty(n, dtype=torch.uint8, device="cuda") if with_ok else None)
        cov, sigma, ok = out
        _check(self._lib.target_batch_crossing_cov_dev(self._h, float(t1), _dp(origin), float(radius), ptr(delta), ptr(slots), n,
                                                       float(sigma_r_max), float(sigma_t_max), ptr(cov), ptr(sigma), ptr(ok)),
               "target_batch_crossing_cov_dev")
        return cov, sigma, ok

    def associate(self, det, dt, gate=float("inf"), rounds=8, out=None, cell=None):
        """Pair a frame of unlabelled detections with this batch's targets on the device (target_batch_associate[_dev]): the cost
        is the position-only Mahalanobis distance d2 against the filter's own predicted position and innovation covariance at
        dt, pairs with d2 <= gate are candidates, matching runs `rounds` rounds of mutual best (info[2] = 1: the greedy
        global-nearest-neighbour result).  det: [M, 7] rows [x y z qx qy qz qw].
        A CUDA double tensor: the device form, on the batch's stream, no host wait.  Returns a SimpleNamespace of CUDA tensors:
        meas [7, size] (batch precision) and has_meas [size] uint8 -- feed them to step(dt, r.meas, r.has_meas) --, det_of_slot
        [size] int32, d2_of_slot [size], slot_of_det [M] int32, d2_of_det [M], info [4] int32 = (matched, rounds_run, settled, 0).
        out: such a namespace to write into (a call with the same tensors allocates nothing and may be captured in a graph).
        A host array: the host form.  Returns a SimpleNamespace of meas / has_meas (CUDA, as above) and NumPy arrays ids_of_det
        [M] uint32 (0xffffffff: none), slot_of_det, d2_of_det, unmatched (ascending detection indices), info, and matched.
        cell: None pairs by brute force over all (target, detection) pairs (M <= 65536).  A positive float takes the grid form
        (target_batch_associate_grid[_dev]; M <= TARGET_ASSOC_GRID_MAX_DETECTIONS): cubic cells of that edge, in the unit of the
        positions; gate must then be finite, a pair must also lie in the gate's bounding box, and info[3] is the number of
        wide slots -- targets whose box exceeds a cell and that are therefore paired by brute force: cell is too small for them."""
        grid = () if cell is None else (float(cell),)
        sfx = "" if cell is None else "_grid"
        import torch
        from types import SimpleNamespace
        n = self.size
        if out is None:
            out = SimpleNamespace(meas=torch.empty((7, max(n, 1)), dtype=self.torch_dtype(), device="cuda"),
                                  has_meas=torch.empty(max(n, 1), dtype=torch.uint8, device="cuda"))
        ld = out.meas.stride(0)
        if isinstance(det, torch.Tensor) and det.is_cuda:
            assert det.dtype == torch.float64 and det.dim() == 2 and det.shape[1] == 7 and det.is_contiguous()
            M = int(det.shape[0])
            if not hasattr(out, "info"):
                out.det_of_slot = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
                out.d2_of_slot = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
                out.slot_of_det = torch.empty(M, dtype=torch.int32, device="cuda")
                out.d2_of_det = torch.empty(M, dtype=torch.float64, device="cuda")
                out.info = torch.empty(4, dtype=torch.int32, device="cuda")
            name = "target_batch_associate%s_dev" % sfx
            _check(getattr(self._lib, name)(self._h, float(dt), det.data_ptr(), M, float(gate), int(rounds), *grid, out.meas.data_ptr(), ld,
                                            out.has_meas.data_ptr(), out.det_of_slot.data_ptr(), out.d2_of_slot.data_ptr(),
                                            out.slot_of_det.data_ptr(), out.d2_of_det.data_ptr(), out.info.data_ptr()), name)
            return out
        det = np.ascontiguousarray(np.asarray(det, dtype=np.float64).reshape(-1, 7))
        M = det.shape[0]
        out.ids_of_det = np.empty(M, dtype=np.uint32)
        out.slot_of_det = np.empty(M, dtype=np.int32)
        out.d2_of_det = np.empty(M)
        unmatched = np.empty(max(M, 1), dtype=np.int64)
        nu = C.c_long(0)
        out.info = np.zeros(4, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        name = "target_batch_associate%s" % sfx
        out.matched = _check(getattr(self._lib, name)(
            self._h, float(dt), _dp(det), M, float(gate), int(rounds), *grid, out.meas.data_ptr(), ld, out.has_meas.data_ptr(),
            out.ids_of_det.ctypes.data_as(capi.c_uint_p), ip(out.slot_of_det), _dp(out.d2_of_det),
            unmatched.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nu), ip(out.info)), name)
        out.unmatched = unmatched[:nu.value].copy()
        return out

    def pack_meas(self, meas_aos, out=None):
        """CUDA double [n,7] (the reference's row layout) -> SoA [7,n] in the batch precision."""
        import torch
        n = meas_aos.shape[0]
        assert meas_aos.is_cuda and meas_aos.dtype == torch.float64 and meas_aos.is_contiguous()
        if out is None:
            out = torch.empty((7, n), dtype=self.torch_dtype(), device="cuda")
        _check(self._lib.target_batch_pack_meas_dev(self._h, meas_aos.data_ptr(), n, out.data_ptr(), out.stride(0)),
               "target_batch_pack_meas_dev")
        return out


class MeasurementIngest:
    """The ROS node's mailbox / has-measurement / expiry policy (RosTargetManager::update) over a manager."""

    def __init__(self, manager, type=None, Q=None, R=None, P0=None, expiration_time=None, token=None):
        self._lib = manager._lib
        self._mgr = manager
        if Q is None:
            self._h = self._lib.target_ingest_new(manager.handle, 0, None, None, None)
        else:
            n, m = MODEL_DIMS[int(type)]
            self._h = self._lib.target_ingest_new(manager.handle, int(type), _dp(_d(Q, (n, n))), _dp(_d(R, (m, m))), _dp(_d(P0, (n, n))))
        if not self._h:
            raise RuntimeError("target_ingest_new failed: %s" % capi.last_error())
        if expiration_time is not None:
            self._lib.target_ingest_set_expiration_time(self._h, float(expiration_time))
        if token is not None:
            self._lib.target_ingest_set_token_name(self._h, token.encode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.target_ingest_delete(self._h)
            self._h = None

    def push(self, id, stamp, pose):
        _check(self._lib.target_ingest_push(self._h, int(id), float(stamp), _dp(_d(pose, (7,)))), "target_ingest_push")

    def push_named(self, frame, stamp, pose):
        return self._lib.target_ingest_push_named(self._h, frame.encode(), float(stamp), _dp(_d(pose, (7,))))

    def tick(self, dt, now, capacity=4096):
        ids = np.zeros(capacity, dtype=np.uint32)
        poses = np.zeros((capacity, 7))
        n = _check(self._lib.target_ingest_tick(self._h, float(dt), float(now), ids.ctypes.data_as(capi.c_uint_p), _dp(poses),
                                                capacity), "target_ingest_tick")
        return ids[:n].copy(), poses[:n].copy()


class TargetManager:
    """ctypes mirror of the reference TargetManager; dtype 'f64' (reference precision) or 'f32'."""

    def __init__(self, file=None, dtype="f64", lanes_per_target=0, devices=None, shared_axes=None, uniform_tiles=None):
        """devices: HIP device indices, one shard each (repeats allowed; target_manager_set_devices).  None: unsharded.
        shared_axes: False keeps this manager's batches out of the shared-axes storage form (target_manager_set_shared_axes);
        None: the default (on unless TE_SHARED_AXES=0).
        uniform_tiles: False keeps its shared-axes batches from sharing covariance words between the targets of a tile
        (target_manager_set_uniform_tiles); None: the default (on unless TE_UNIFORM_TILES=0)."""
        self._lib = capi.lib()
        f = None if file is None else str(file).encode()
        self._h = self._lib.target_manager_new_ex(f, DTYPES[dtype], int(lanes_per_target))
        if not self._h:
            raise RuntimeError("target_manager_new failed: %s" % capi.last_error())
        self.dtype = dtype
        if shared_axes is not None:
            _check(self._lib.target_manager_set_shared_axes(self._h, 1 if shared_axes else 0), "target_manager_set_shared_axes")
        if uniform_tiles is not None:
            _check(self._lib.target_manager_set_uniform_tiles(self._h, 1 if uniform_tiles else 0), "target_manager_set_uniform_tiles")
        if devices is not None:
            try:
                self.set_devices(devices)
            except Exception:
                self.close()
                raise

    # ---- several devices (target_manager_set_devices) -----------------------------------------
    def set_devices(self, devices):
        devs = np.ascontiguousarray(np.asarray(list(devices), dtype=np.int32))
        _check(self._lib.target_manager_set_devices(self._h, devs.ctypes.data_as(C.POINTER(C.c_int)), len(devs)),
               "target_manager_set_devices")

    @property
    def num_shards(self):
        return self._lib.target_manager_num_shards(self._h)

    def shard_device(self, k):
        return self._lib.target_manager_shard_device(self._h, int(k))

    def shard_of(self, id):
        return self._lib.target_manager_shard_of(self._h, int(id))

    def batch_shard(self, i):
        return self._lib.target_manager_batch_shard(self._h, int(i))

    def set_shard_stream(self, k, stream_ptr):
        _check(self._lib.target_manager_set_shard_stream(self._h, int(k), stream_ptr), "target_manager_set_shard_stream")

    def get_est_all_by_id(self, out=None):
        """pose7 of every target in ascending id order (get_available_targets).  out: a torch tensor [>= size, 7] of doubles
        on the GPU or in pinned host memory (filled asynchronously; complete after synchronize()), or None: a numpy array
        (through a pinned staging buffer, synchronised here)."""
        if out is not None:
            import torch
            if out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != 7 or not out.is_contiguous():
                raise ValueError("get_est_all_by_id: out must be a contiguous float64 tensor [rows, 7], got %s %s" % (out.dtype, tuple(out.shape)))
            n = self._lib.target_manager_get_est_all_by_id(self._h, out.data_ptr(), out.shape[0])
            if n < 0:
                raise RuntimeError("target_manager_get_est_all_by_id: %s" % capi.last_error())
            return out[:n]
        import torch
        n = self.size()
        buf = torch.empty((max(n, 1), 7), dtype=torch.float64, pin_memory=True)
        k = self._lib.target_manager_get_est_all_by_id(self._h, buf.data_ptr(), buf.shape[0])
        if k < 0:
            raise RuntimeError("target_manager_get_est_all_by_id: %s" % capi.last_error())
        self.synchronize()
        return buf[:k].numpy().copy()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.target_manager_delete(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    # ---- the reference's per-target calls ---------------------------------------------------
    def init(self, id, dt0, t0, p0, v0=None, a0=None, type=None, Q=None, R=None, P0=None):
        p0 = _d(p0, (7,))
        if type is None:
            assert v0 is None and a0 is None, "the C boundary's init takes a pose only (target_manager_c.h:29)"
            self._lib.target_manager_init(self._h, int(id), float(dt0), _dp(p0), float(t0))
            return
        n, m = MODEL_DIMS[int(type)]
        Q, R, P0 = _d(Q, (n, n)), _d(R, (m, m)), _d(P0, (n, n))
        v0, a0 = _d(v0, (6,)), _d(a0, (6,))
        _check(self._lib.target_manager_init_typed(self._h, int(type), int(id), float(dt0), float(t0), _dp(Q), _dp(R),
                                                    _dp(P0), _dp(p0), _dp(v0), _dp(a0)), "target_manager_init_typed")

    def update(self, id, dt, meas=None):
        if meas is None:
            self._lib.target_manager_update(self._h, int(id), float(dt))
        else:
            meas = _d(meas, (7,))
            self._lib.target_manager_update_meas(self._h, int(id), float(dt), _dp(meas))

    def update_all(self, dt):
        _check(self._lib.target_manager_update_all(self._h, float(dt)), "target_manager_update_all")

    def erase(self, id):
        return bool(_check(self._lib.target_manager_erase(self._h, int(id)), "target_manager_erase"))

    def erase_batch(self, ids):
        ids, idp = _ids(ids)
        return self._lib.target_manager_erase_batch(self._h, idp, len(ids))

    def _get1(self, fn, id, w):
        out = np.full(w, np.nan)
        ok = fn(self._h, int(id), _dp(out))
        return bool(ok), out

    def getTargetPose(self, id):
        return self._get1(self._lib.target_manager_get_est_pose, id, 7)

    def getTargetTwist(self, id):
        return self._get1(self._lib.target_manager_get_est_twist, id, 6)

    def getTargetAcceleration(self, id):
        return self._get1(self._lib.target_manager_get_est_acceleration, id, 6)

    def getNumberMeasurements(self, id):
        return self._lib.target_manager_get_n_measurements(self._h, int(id))

    def getRejectionRun(self, id):
        """The target's run of consecutive gate rejections (step_sequence(..., reacquire=)), or None for an unknown id."""
        rc = self._lib.target_manager_get_rejection_run(self._h, int(id))
        return rc if rc >= 0 else None

    def getAvailableTargets(self):
        n = self._lib.target_manager_size(self._h)
        out = np.empty(max(n, 1), dtype=np.uint32)
        n = self._lib.target_manager_get_available_targets(self._h, out.ctypes.data_as(capi.c_uint_p), n)
        return out[:n]

    def getTime(self, id):
        t = C.c_double()
        rc = self._lib.target_manager_get_time(self._h, int(id), C.byref(t))
        return t.value if rc == 0 else None

    def log(self):
        self._lib.target_manager_log(self._h)

    def set_log_directory(self, path):
        _check(self._lib.target_manager_set_log_directory(self._h, None if path is None else str(path).encode()),
               "target_manager_set_log_directory")

    def set_log_targets(self, ids):
        ids, idp = _ids(ids if ids is not None else [])
        _check(self._lib.target_manager_set_log_targets(self._h, idp, len(ids)), "target_manager_set_log_targets")

    def set_keep_measurement(self, on=True):
        _check(self._lib.target_manager_set_keep_measurement(self._h, 1 if on else 0), "target_manager_set_keep_measurement")

    # TargetInterface getters reached through getTarget(id)-> in the reference (target_interface.hpp:94-148)
    def getMeasuredPose(self, id):
        return self._get1(self._lib.target_manager_get_measured_pose, id, 7)

    def getPeriodEstimate(self, id):
        p = C.c_double(float("nan"))
        ok = self._lib.target_manager_get_period_estimate(self._h, int(id), C.byref(p))
        return p.value if ok else None

    def getEstimatedTransform(self, id):
        ok, T = self._get1(self._lib.target_manager_get_estimated_transform, id, 16)
        return bool(ok), T.reshape(4, 4)

    def getN(self, id):
        return self._lib.target_manager_get_n(self._h, int(id))

    def getM(self, id):
        return self._lib.target_manager_get_m(self._h, int(id))

    def getModelMatrices(self, id):
        """(Q, R, P0) the target was created with (getEstimator()->getQ / getR / getP0), or None for an unknown id."""
        n, m = self.getN(id), self.getM(id)
        if n <= 0:
            return None
        Q, R, P0 = np.empty((n, n)), np.empty((m, m)), np.empty((n, n))
        ok = self._lib.target_manager_get_model_matrices(self._h, int(id), _dp(Q), _dp(R), _dp(P0))
        return (Q, R, P0) if ok else None

    def size(self):
        return self._lib.target_manager_size(self._h)

    def synchronize(self):
        _check(self._lib.target_manager_synchronize(self._h), "target_manager_synchronize")

    def set_stream(self, stream_ptr):
        _check(self._lib.target_manager_set_stream(self._h, stream_ptr), "target_manager_set_stream")

    # ---- batched extension ---------------------------------------------------------------------
    def init_batch(self, ids, dt0, t0, p0, v0=None, a0=None, type=None, Q=None, R=None, P0=None):
        ids, idp = _ids(ids)
        n = len(ids)
        p0, v0, a0 = _d(p0, (n, 7)), _d(v0, (n, 6)), _d(a0, (n, 6))
        if type is None:
            return _check(self._lib.target_manager_init_batch(self._h, idp, n, float(dt0), float(t0), _dp(p0), _dp(v0),
                                                              _dp(a0)), "target_manager_init_batch")
        ns, m = MODEL_DIMS[int(type)]
        Q, R = _d(Q, (ns, ns)), _d(R, (m, m))
        P0 = _d(P0)
        per = 1 if P0.ndim == 3 else 0
        return _check(self._lib.target_manager_init_batch_typed(
            self._h, int(type), idp, n, float(dt0), float(t0), _dp(Q), _dp(R), _dp(np.ascontiguousarray(P0)), per,
            _dp(p0), _dp(v0), _dp(a0)), "target_manager_init_batch_typed")

    def init_batch_classes(self, ids, dt0, t0, p0, type, Q, R, P0, class_of, v0=None, a0=None):
        """n targets with per-class parameters: Q [n_classes, ns, ns], R [n_classes, m, m], P0 [n_classes, ns, ns],
        class_of [n] (the class of every target).  All classes of one layout share one batch (one launch per tick)."""
        ids, idp = _ids(ids)
        n = len(ids)
        ns, m = MODEL_DIMS[int(type)]
        Q, R, P0 = _d(Q), _d(R), _d(P0)
        nc = Q.shape[0]
        assert Q.shape == (nc, ns, ns) and R.shape == (nc, m, m) and P0.shape == (nc, ns, ns)
        class_of = np.ascontiguousarray(class_of, dtype=np.uint32)
        assert class_of.shape == (n,) and (class_of < nc).all()
        p0, v0, a0 = _d(p0, (n, 7)), _d(v0, (n, 6)), _d(a0, (n, 6))
        return _check(self._lib.target_manager_init_batch_classes(
            self._h, int(type), idp, n, float(dt0), float(t0), nc, _dp(Q), _dp(R), _dp(P0), class_of.ctypes.data_as(capi.c_uint_p),
            _dp(p0), _dp(v0), _dp(a0)), "target_manager_init_batch_classes")

    def set_update_gate(self, nis_max, max_rejects=-1, type=-1):
        """The sticky update policy of the by-id paths (target_manager_set_update_gate): from now on update(id, dt, meas),
        update_batch and the ingest tick fold a measurement in iff its NIS <= nis_max (0: no gate, the default) and, with
        max_rejects >= 0, keep every target's run of consecutive rejections (getRejectionRun) and re-initialise a target from
        the measurement of its max_rejects-th consecutive rejection (0: count only; -1: gate only).  type: a model type (a name
        of MODEL_TYPES or its number), or -1 = every model."""
        _check(self._lib.target_manager_set_update_gate(self._h, _model_type(type), float(nis_max), int(max_rejects)),
               "target_manager_set_update_gate")

    setUpdateGate = set_update_gate

    def get_update_gate(self, type):
        """(nis_max, max_rejects) of a model type's policy."""
        g, k = C.c_double(0.0), C.c_int(-1)
        _check(self._lib.target_manager_get_update_gate(self._h, _model_type(type), C.byref(g), C.byref(k)), "target_manager_get_update_gate")
        return g.value, k.value

    getUpdateGate = get_update_gate

    def update_gate_served(self, type):
        """True / False: by-id updates of this model's batches would be served under a policy; None: no such batch yet."""
        rc = self._lib.target_manager_update_gate_served(self._h, _model_type(type))
        return None if rc < 0 else bool(rc)

    def update_batch(self, ids, dt, meas=None, has_meas=None, gated=False):
        """gated=True: target_manager_update_meas_batch_gated -> (done, nis [n] float64, event [n] uint8), per entry in the
        caller's order: nis -1 = no measurement judged on the entry, -2 = unknown id; event as the re-acquisition table."""
        ids, idp = _ids(ids)
        n = len(ids)
        meas = _d(meas, (n, 7))
        hp = None
        if has_meas is not None:
            has_meas = np.ascontiguousarray(has_meas, dtype=np.uint8)
            hp = has_meas.ctypes.data_as(capi.c_ubyte_p)
        if gated:
            nis = np.zeros(max(n, 1), dtype=np.float64)
            event = np.zeros(max(n, 1), dtype=np.uint8)
            done = _check(self._lib.target_manager_update_meas_batch_gated(self._h, idp, n, float(dt), _dp(meas), hp, _dp(nis),
                                                                           event.ctypes.data_as(capi.c_ubyte_p)),
                          "target_manager_update_meas_batch_gated")
            return done, nis[:n], event[:n]
        return _check(self._lib.target_manager_update_meas_batch(self._h, idp, n, float(dt), _dp(meas), hp),
                      "target_manager_update_meas_batch")

    def get_est_batch(self, ids, t1=None):
        ids, idp = _ids(ids)
        n = len(ids)
        pose, twist, acc = np.full((n, 7), np.nan), np.full((n, 6), np.nan), np.full((n, 6), np.nan)
        found = np.zeros(n, dtype=np.uint8)
        fp = found.ctypes.data_as(capi.c_ubyte_p)
        if t1 is None:
            _check(self._lib.target_manager_get_est_batch(self._h, idp, n, _dp(pose), _dp(twist), _dp(acc), fp),
                   "target_manager_get_est_batch")
        else:
            _check(self._lib.target_manager_get_est_at_batch(self._h, idp, n, float(t1), _dp(pose), _dp(twist), _dp(acc),
                                                             fp), "target_manager_get_est_at_batch")
        return pose, twist, acc, found.astype(bool)

    def get_state_batch(self, ids):
        ids, idp = _ids(ids)
        n = len(ids)
        x = np.empty((n, 18)); P = np.empty((n, 18 * 18))
        ns = _check(self._lib.target_manager_get_state_batch(self._h, idp, n, _dp(x), _dp(P)),
                    "target_manager_get_state_batch")
        return (x.reshape(-1)[:n * ns].reshape(n, ns).copy(),
                P.reshape(-1)[:n * ns * ns].reshape(n, ns, ns).copy())

    def intersection_time(self, id, t1, origin, radius):
        origin = _d(origin, (3,))
        return self._lib.target_manager_get_intersection_time_with_sphere(self._h, int(id), float(t1), _dp(origin), float(radius))

    def intersection_pose(self, id, t1, origin, radius):
        origin = _d(origin, (3,))
        pose = np.zeros(7)
        d = C.c_double()
        ok = self._lib.target_manager_get_intersection_pose_with_sphere(self._h, int(id), float(t1), _dp(origin), float(radius),
                                                                         _dp(pose), C.byref(d))
        return bool(ok), pose, d.value

    def intersect_batch(self, ids, t1, origin, radius):
        ids, idp = _ids(ids)
        n = len(ids)
        origin = _d(origin, (3,))
        delta = np.empty(n); pose = np.empty((n, 7)); found = np.zeros(n, dtype=np.uint8)
        _check(self._lib.target_manager_intersect_sphere_batch(self._h, idp, n, float(t1), _dp(origin), float(radius),
                                                               _dp(delta), _dp(pose), found.ctypes.data_as(capi.c_ubyte_p)),
               "target_manager_intersect_sphere_batch")
        return delta, pose, found.astype(bool)

    def intersect_converged_batch(self, ids, t1, pos_th, ang_th, origin, radius, filters_length=250):
        """IntersectionSolver::getIntersectionPoseWithSphere incl. its convergence gate (one gate per target):
        returns converged [n] bool, pose [n,7], delta [n], filtered errors [n,2]."""
        ids, idp = _ids(ids)
        n = len(ids)
        origin = _d(origin, (3,))
        delta = np.empty(n); pose = np.empty((n, 7)); filt = np.empty((n, 2))
        conv = np.zeros(n, dtype=np.uint8); found = np.zeros(n, dtype=np.uint8)
        _check(self._lib.target_manager_intersect_sphere_converged_batch(
            self._h, idp, n, float(t1), float(pos_th), float(ang_th), _dp(origin), float(radius), int(filters_length),
            _dp(delta), _dp(pose), conv.ctypes.data_as(capi.c_ubyte_p), found.ctypes.data_as(capi.c_ubyte_p), _dp(filt)),
            "target_manager_intersect_sphere_converged_batch")
        return conv.astype(bool), pose, delta, filt

    def step_fused_all(self, dt, meas, has_meas=None, n_ticks=None, poses=None, innov=None, gate=None, reacquire=None):
        """A temporally fused replay of every batch (target_manager_step_fused_all): for every batch, bit for bit, what
        Batch.step_fused(dt, meas[i], ..., innov=, gate=, reacquire=) leaves -- as ONE launch per device where
        fused_all_served() is 1, otherwise batch by batch inside the call.
        meas: one CUDA tensor [ticks, 7, ld] per batch (batches() order), or None for a batch that only predicts; has_meas, poses,
        innov, gate and reacquire per batch with step_sequence_all's conventions.  n_ticks: the ticks of the call (by default those
        of the first tensor); the tensors are read linearly, never as rings.
        dt: a number, or a sequence / array with one time step per tick (target_manager_step_fused_all_dt)."""
        nb = len(meas)          # the library checks it against the number of batches
        first = next((t for t in meas if t is not None), None)
        ticks = int(n_ticks) if n_ticks is not None else (first.shape[0] if first is not None else 0)
        sched = _dt_schedule(dt, ticks)
        specs = (capi.BatchSequence * max(nb, 1))()
        for i, t in enumerate(meas):
            if t is not None:
                assert t.is_cuda and t.dim() == 3 and t.shape[0] >= ticks and t.shape[1] == 7 and (t.shape[2] == 1 or t.stride(2) == 1)
                specs[i].meas_dev, specs[i].tick_stride, specs[i].ld = t.data_ptr(), t.stride(0), t.stride(1)
            if has_meas is not None and has_meas[i] is not None:
                h = has_meas[i]
                assert h.is_cuda and h.dim() == 2 and h.element_size() == 1 and h.shape[0] >= ticks
                specs[i].has_meas_dev, specs[i].has_stride = h.data_ptr(), h.stride(0)
        bs = self.batches()
        sizes = [bs[i].size if i < len(bs) else 0 for i in range(nb)]
        pss = iss = gs = rqs = None
        if poses is not None:
            assert len(poses) == nb, "one pose stream (or None) per batch"
            pss = (capi.PoseStream * max(nb, 1))()
            for i in range(nb):
                if poses[i] is not None:
                    pss[i] = _pose_stream(poses[i], sizes[i], ticks)
        if innov is not None:
            assert len(innov) == nb, "one stream (or None) per batch"
            iss = (capi.InnovStream * max(nb, 1))()
            for i in range(nb):
                if innov[i] is not None:
                    iss[i] = _innov_stream(innov[i], sizes[i], bs[i].meas_dim if i < len(bs) else 3, ticks)
        if gate is not None:
            per = list(gate) if isinstance(gate, (list, tuple)) else [gate] * nb
            assert len(per) == nb, "one gate (or None) per batch"
            gs = (C.c_double * max(nb, 1))(*[0.0 if g is None else float(g) for g in per])
        if reacquire is not None:
            per = list(reacquire) if isinstance(reacquire, list) else [reacquire] * nb
            assert len(per) == nb, "one re-acquisition policy (or None) per batch"
            rqs = (capi.Reacquire * max(nb, 1))()
            for i in range(nb):
                rqs[i] = _reacquire(per[i], sizes[i], ticks)
        if sched is not None:
            _check(self._lib.target_manager_step_fused_all_dt(
                self._h, ticks, sched.ctypes.data_as(capi.c_double_p), C.cast(specs, C.c_void_p), pss, iss, gs, rqs, nb),
                "target_manager_step_fused_all_dt")
        else:
            _check(self._lib.target_manager_step_fused_all(self._h, ticks, float(dt), C.cast(specs, C.c_void_p), pss, iss, gs, rqs, nb),
                   "target_manager_step_fused_all")

    def fused_all_served(self, gated=False, scheduled=False):
        """1: step_fused_all would be one launch per device as the batches are now -- gated: with a stream (innov=, gate=) on every
        batch; scheduled: with a time step per tick --; 0: served batch by batch inside the call
        (target_manager_step_fused_all_served)."""
        return _check(self._lib.target_manager_step_fused_all_served(self._h, 1 if gated else 0, 1 if scheduled else 0),
                      "target_manager_step_fused_all_served")

    def step_sequence_all(self, dt, meas, has_meas=None, query=None, use_graph=True, n_ticks=None, poses=None, innov=None, gate=None,
                          reacquire=None):
        """meas: one CUDA tensor [ticks, 7, ld] per batch (batches() order): `ticks` ticks of every batch -- ONE launch per
        tick for all of them where population_tick() holds, otherwise a launch per batch (recorded: one graph branch per
        batch) -- replayed from a recorded hipGraph (use_graph) or eagerly.  query =
        (origin[3], radius, deltas, poses) adds the own-time sphere query of every target after every step;
        deltas[i] [size] and poses[i] [size, 7] (or None) are CUDA double tensors, overwritten every tick.
        poses: one pose stream per batch (a tensor as for Batch.step_sequence, or None for a batch without one): every
        target's pose after every tick (target_manager_step_sequence_all_poses).
        innov: one innovation stream per batch ((nis, nu_or_None) as for Batch.step_sequence, or None for a batch without one):
        every target's NIS and innovations of every tick (target_manager_step_sequence_all_innov).
        gate: the NIS validation gate of every batch (a number) or one per batch (a list; 0 or None: that batch has none), as for
        Batch.step_sequence (target_manager_step_sequence_all_gated).
        reacquire: the re-acquisition policy (K, events_or_None) of every batch (one tuple) or one per batch (a list; None: that
        batch has none), as for Batch.step_sequence (target_manager_step_sequence_all_reacquire).
        dt: a number, or a sequence / array with one time step per tick (target_manager_step_sequence_all_dt): tick s of every
        batch runs with dt[s]."""
        nb = len(meas)          # the library checks it against the number of batches
        ring = meas[0].shape[0] if nb else 0
        ticks = ring if n_ticks is None else int(n_ticks)      # n_ticks > ring: the tensors are rings (tick s reads s % ring)
        sched = _dt_schedule(dt, ticks)
        specs = (capi.BatchSequence * max(nb, 1))()
        for i, t in enumerate(meas):
            assert t.is_cuda and t.dim() == 3 and t.shape[0] == ring and t.shape[1] == 7 and (t.shape[2] == 1 or t.stride(2) == 1)
            specs[i].meas_dev, specs[i].tick_stride, specs[i].ld = t.data_ptr(), t.stride(0), t.stride(1)
            specs[i].ring_ticks = ring if ticks != ring else 0
            if has_meas is not None and has_meas[i] is not None:
                h = has_meas[i]
                assert h.is_cuda and h.dim() == 2 and h.element_size() == 1 and h.shape[0] == ring
                specs[i].has_meas_dev, specs[i].has_stride = h.data_ptr(), h.stride(0)
        origin, radius = None, 0.0
        if query is not None:
            origin, radius, deltas, qposes = query
            origin = _d(origin, (3,))
            for i in range(nb):
                specs[i].delta_dev = deltas[i].data_ptr()
                specs[i].pose_dev = None if qposes is None or qposes[i] is None else qposes[i].data_ptr()
        if sched is not None:   # the most general form: streams, gates and policies as given, or NULL
            bs = self.batches()
            sizes = [bs[i].size if i < len(bs) else 0 for i in range(nb)]
            pss = iss = gs = rqs = None
            if poses is not None:
                assert len(poses) == nb, "one pose stream (or None) per batch"
                pss = (capi.PoseStream * max(nb, 1))()
                for i in range(nb):
                    if poses[i] is not None:
                        pss[i] = _pose_stream(poses[i], sizes[i], ticks)
            if innov is not None:
                assert len(innov) == nb, "one stream (or None) per batch"
                iss = (capi.InnovStream * max(nb, 1))()
                for i in range(nb):
                    if innov[i] is not None:
                        iss[i] = _innov_stream(innov[i], sizes[i], bs[i].meas_dim if i < len(bs) else 3, ticks)
            if gate is not None:
                per = list(gate) if isinstance(gate, (list, tuple)) else [gate] * nb
                assert len(per) == nb, "one gate (or None) per batch"
                gs = (C.c_double * max(nb, 1))(*[0.0 if g is None else float(g) for g in per])
            if reacquire is not None:
                per = list(reacquire) if isinstance(reacquire, list) else [reacquire] * nb
                assert len(per) == nb, "one re-acquisition policy (or None) per batch"
                rqs = (capi.Reacquire * max(nb, 1))()
                for i in range(nb):
                    rqs[i] = _reacquire(per[i], sizes[i], ticks)
            _check(self._lib.target_manager_step_sequence_all_dt(
                self._h, ticks, sched.ctypes.data_as(capi.c_double_p), C.cast(specs, C.c_void_p), pss, iss, gs, rqs, nb,
                0 if query is None else 1, None if origin is None else _dp(origin), float(radius), int(use_graph)),
                "target_manager_step_sequence_all_dt")
            return
        gates = None
        if reacquire is not None and gate is None:
            gate = 0.0   # (a policy without a gate is the library's to refuse)
        if gate is not None:
            per = list(gate) if isinstance(gate, (list, tuple)) else [gate] * nb
            assert len(per) == nb, "one gate (or None) per batch"
            gates = (C.c_double * max(nb, 1))(*[0.0 if g is None else float(g) for g in per])
            if innov is None:
                innov = [None] * nb
        if innov is not None:
            assert len(innov) == nb and (poses is None or len(poses) == nb), "one stream (or None) per batch"
            bs = self.batches()
            pss = (capi.PoseStream * max(nb, 1))()
            iss = (capi.InnovStream * max(nb, 1))()
            for i in range(nb):
                size = bs[i].size if i < len(bs) else 0
                if poses is not None and poses[i] is not None:
                    pss[i] = _pose_stream(poses[i], size, ticks)
                if innov[i] is not None:
                    iss[i] = _innov_stream(innov[i], size, bs[i].meas_dim if i < len(bs) else 3, ticks)
            if reacquire is not None:
                per = list(reacquire) if isinstance(reacquire, list) else [reacquire] * nb
                assert len(per) == nb, "one re-acquisition policy (or None) per batch"
                rqs = (capi.Reacquire * max(nb, 1))()
                for i in range(nb):
                    rqs[i] = _reacquire(per[i], bs[i].size if i < len(bs) else 0, ticks)
                _check(self._lib.target_manager_step_sequence_all_reacquire(
                    self._h, ticks, float(dt), C.cast(specs, C.c_void_p), pss, iss, gates, rqs, nb, 0 if query is None else 1,
                    None if origin is None else _dp(origin), float(radius), int(use_graph)), "target_manager_step_sequence_all_reacquire")
                return
            if gates is not None:
                _check(self._lib.target_manager_step_sequence_all_gated(
                    self._h, ticks, float(dt), C.cast(specs, C.c_void_p), pss, iss, gates, nb, 0 if query is None else 1,
                    None if origin is None else _dp(origin), float(radius), int(use_graph)), "target_manager_step_sequence_all_gated")
                return
            _check(self._lib.target_manager_step_sequence_all_innov(
                self._h, ticks, float(dt), C.cast(specs, C.c_void_p), pss, iss, nb, 0 if query is None else 1,
                None if origin is None else _dp(origin), float(radius), int(use_graph)), "target_manager_step_sequence_all_innov")
            return
        if poses is not None:
            assert len(poses) == nb, "one pose stream (or None) per batch"
            bs = self.batches()
            pss = (capi.PoseStream * max(nb, 1))()
            for i, p in enumerate(poses):
                if p is not None:
                    pss[i] = _pose_stream(p, bs[i].size if i < len(bs) else 0, ticks)
            _check(self._lib.target_manager_step_sequence_all_poses(
                self._h, ticks, float(dt), C.cast(specs, C.c_void_p), pss, nb, 0 if query is None else 1,
                None if origin is None else _dp(origin), float(radius), int(use_graph)), "target_manager_step_sequence_all_poses")
            return
        _check(self._lib.target_manager_step_sequence_all(
            self._h, ticks, float(dt), C.cast(specs, C.c_void_p), nb, 0 if query is None else 1,
            None if origin is None else _dp(origin), float(radius), int(use_graph)), "target_manager_step_sequence_all")

    def select_soonest(self, per_batch, ok=None, k=8, window=(0.0, float("inf")), want_pose=True, device=False, out=None):
        """The k soonest sphere crossings of the whole manager (target_manager_select_soonest[_dev]).  per_batch: the per-batch
        description step_sequence_all's query= uses -- (origin, radius, deltas, poses), of which only the last two are read -- or
        (deltas, poses): deltas[i] [size_i] and poses[i] [size_i, 7] (poses or an entry None) CUDA doubles per batch in batches()
        order; a None delta skips the batch.  ok: one CUDA uint8 / bool mask (or None) per batch, or None.  Order: (delta, batch
        index, slot).  want_pose=False leaves the poses alone.
        device=False -> (count, ids [k], batch [k], slots [k], delta [k], pose [k, 7] or None) NumPy arrays, the shards' rows merged
        on the host.  device=True (a manager on one device only) -> (count [1], batch [k], slots [k], delta [k], pose or None) CUDA
        tensors, no host wait.  out: the output arrays to use, in the order returned (without count for device=False)."""
        import torch
        deltas, poses = per_batch[-2], per_batch[-1]
        nb = len(deltas)
        k = int(k)
        ptr = lambda t: None if t is None else t.data_ptr()
        specs = (capi.BatchSequence * max(nb, 1))()
        for i in range(nb):
            specs[i].delta_dev = ptr(deltas[i])
            specs[i].pose_dev = None if poses is None else ptr(poses[i])
        oks = None
        if ok is not None:
            assert len(ok) == nb, "one mask (or None) per batch"
            oks = (C.c_void_p * max(nb, 1))(*[ptr(o) for o in ok])
        with_pose = want_pose and poses is not None and any(p is not None for p in poses)
        kk = max(k, 1)
        if device:
            if out is None:
                out = (torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(kk, dtype=torch.int32, device="cuda"),
                       torch.empty(kk, dtype=torch.int32, device="cuda"), torch.empty(kk, dtype=torch.float64, device="cuda"),
                       torch.empty((kk, 7), dtype=torch.float64, device="cuda") if with_pose else None)
            cnt, bo, so, do, po = out
            _check(self._lib.target_manager_select_soonest_dev(self._h, C.cast(specs, C.c_void_p), nb, oks, float(window[0]), float(window[1]), k,
                                                               ptr(bo), ptr(so), ptr(do), ptr(po), ptr(cnt)), "target_manager_select_soonest_dev")
            return cnt, bo, so, do, po
        if out is None:
            out = (np.empty(kk, dtype=np.uint32), np.empty(kk, dtype=np.int32), np.empty(kk, dtype=np.int32), np.empty(kk),
                   np.empty((kk, 7)) if with_pose else None)
        ids, bo, so, do, po = out
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
        count = _check(self._lib.target_manager_select_soonest(self._h, C.cast(specs, C.c_void_p), nb, oks, float(window[0]), float(window[1]), k,
                                                               None if ids is None else ids.ctypes.data_as(capi.c_uint_p), ip(bo), ip(so),
                                                               _dp(do), _dp(po)), "target_manager_select_soonest")
        return count, ids, bo, so, do, po

    def crossing_cov(self, batch, slots, delta, origin=None, radius=0.0, t1=float("nan"), sigma_r_max=float("inf"),
                     sigma_t_max=float("inf"), want_ok=None, out=None):
        """Position covariance and time spread (target_manager_crossing_cov_dev) of the rows select_soonest(device=True) left on
        the device: batch / slots CUDA int32 [n], delta CUDA doubles [n], n <= 8192; a manager on one device only, no host wait.
        Returns (cov [n, 6], sigma [n, 2] or None, ok [n] uint8 or None) CUDA tensors as Batch.crossing_cov; rows of batch -1 or
        slot -1 are cov 0, sigma (-1, -1), ok 0."""
        import torch
        n = int(delta.shape[0])
        origin = _d(origin, (3,))
        ptr = lambda t: None if t is None else t.data_ptr()
        if out is None:
            with_ok = (origin is not None) if want_ok is None else bool(want_ok)
            out = (torch.empty((n, 6), dtype=torch.float64, device="cuda"),
                   None if origin is None else torch.empty((n, 2), dtype=torch.float64, device="cuda"),
                   torch.empty(n, dtype=torch.uint8, device="cuda") if with_ok else None)
        cov, sigma, ok = out
        _check(self._lib.target_manager_crossing_cov_dev(self._h, float(t1), _dp(origin), float(radius), ptr(batch), ptr(slots), ptr(delta), n,
                                                         float(sigma_r_max), float(sigma_t_max), ptr(cov), ptr(sigma), ptr(ok)),
               "target_manager_crossing_cov_dev")
        return cov, sigma, ok

    def crossing_cov_batch(self, ids, delta, origin=None, radius=0.0, t1=float("nan"), sigma_r_max=float("inf"), sigma_t_max=float("inf")):
        """The same by id with host arrays (target_manager_crossing_cov_batch): delta [n] as intersect_batch returned it for the
        same t1, origin and radius.  Any number of ids over any number of devices; the queued one-target steps run first.
        Returns (found count, cov [n, 6], sigma [n, 2] or None, ok [n] bool or None); unknown ids are cov 0, sigma (-1, -1), ok 0."""
        ids, idp = _ids(ids)
        n = len(ids)
        origin = _d(origin, (3,))
        delta = _d(delta, (n,))
        cov = np.empty((n, 6))
        sigma = None if origin is None else np.empty((n, 2))
        ok = None if origin is None else np.zeros(n, dtype=np.uint8)
        found = _check(self._lib.target_manager_crossing_cov_batch(self._h, idp, n, float(t1), _dp(origin), float(radius), _dp(delta),
                                                                   float(sigma_r_max), float(sigma_t_max), _dp(cov), _dp(sigma),
                                                                   None if ok is None else ok.ctypes.data_as(capi.c_ubyte_p)),
                       "target_manager_crossing_cov_batch")
        return found, cov, sigma, None if ok is None else ok.astype(bool)

    def associate(self, det, dt, gate=float("inf"), rounds=8, out=None, cell=None):
        """Pair a frame of unlabelled detections with every target of the manager on the device (target_manager_associate[_dev];
        a manager on one device only): as Batch.associate, a detection picking among the targets of all batches by (d2, batch,
        slot).  det: [M, 7].  A CUDA double tensor: the device form, no host wait.  Returns a SimpleNamespace: meas / has_meas /
        det_of_slot / d2_of_slot are LISTS with one CUDA tensor per batch (batches() order; meas[i] is [1, 7, size_i], the
        one-tick form step_sequence_all(dt, r.meas, r.has_meas, n_ticks=1) reads, has_meas[i] [1, size_i]), slot_of_det /
        batch_of_det / d2_of_det [M] and info [4] CUDA tensors.  out: such a namespace to write into.
        A host array: the host form; the per-detection results come back as NumPy arrays ids_of_det, batch_of_det, slot_of_det,
        d2_of_det, unmatched, info, and matched.
        cell: None = brute force; a positive float = the grid form (target_manager_associate_grid[_dev]), as Batch.associate."""
        import torch
        from types import SimpleNamespace
        grid = () if cell is None else (float(cell),)
        sfx = "" if cell is None else "_grid"
        bs = self.batches()
        nb = len(bs)
        if out is None:
            out = SimpleNamespace(meas=[torch.empty((1, 7, max(b.size, 1)), dtype=b.torch_dtype(), device="cuda") for b in bs],
                                  has_meas=[torch.empty((1, max(b.size, 1)), dtype=torch.uint8, device="cuda") for b in bs],
                                  det_of_slot=[torch.empty(max(b.size, 1), dtype=torch.int32, device="cuda") for b in bs],
                                  d2_of_slot=[torch.empty(max(b.size, 1), dtype=torch.float64, device="cuda") for b in bs])
        per = (capi.AssocOut * max(nb, 1))()
        for i in range(nb):
            per[i].meas_out_dev, per[i].ld = out.meas[i].data_ptr(), out.meas[i].stride(1)
            per[i].has_meas_out_dev = out.has_meas[i].data_ptr()
            per[i].det_of_slot_dev, per[i].d2_of_slot_dev = out.det_of_slot[i].data_ptr(), out.d2_of_slot[i].data_ptr()
        if isinstance(det, torch.Tensor) and det.is_cuda:
            assert det.dtype == torch.float64 and det.dim() == 2 and det.shape[1] == 7 and det.is_contiguous()
            M = int(det.shape[0])
            if not hasattr(out, "info"):
                out.slot_of_det = torch.empty(M, dtype=torch.int32, device="cuda")
                out.batch_of_det = torch.empty(M, dtype=torch.int32, device="cuda")
                out.d2_of_det = torch.empty(M, dtype=torch.float64, device="cuda")
                out.info = torch.empty(4, dtype=torch.int32, device="cuda")
            name = "target_manager_associate%s_dev" % sfx
            _check(getattr(self._lib, name)(self._h, float(dt), det.data_ptr(), M, float(gate), int(rounds), *grid, per, nb,
                                            out.slot_of_det.data_ptr(), out.batch_of_det.data_ptr(), out.d2_of_det.data_ptr(),
                                            out.info.data_ptr()), name)
            return out
        det = np.ascontiguousarray(np.asarray(det, dtype=np.float64).reshape(-1, 7))
        M = det.shape[0]
        out.ids_of_det = np.empty(M, dtype=np.uint32)
        out.batch_of_det = np.empty(M, dtype=np.int32)
        out.slot_of_det = np.empty(M, dtype=np.int32)
        out.d2_of_det = np.empty(M)
        unmatched = np.empty(max(M, 1), dtype=np.int64)
        nu = C.c_long(0)
        out.info = np.zeros(4, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        name = "target_manager_associate%s" % sfx
        out.matched = _check(getattr(self._lib, name)(
            self._h, float(dt), _dp(det), M, float(gate), int(rounds), *grid, per, nb, out.ids_of_det.ctypes.data_as(capi.c_uint_p),
            ip(out.batch_of_det), ip(out.slot_of_det), _dp(out.d2_of_det), unmatched.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nu),
            ip(out.info)), name)
        out.unmatched = unmatched[:nu.value].copy()
        return out

    def lifecycle(self, det, assoc_result, *, max_misses, birth_type=None, first_id, max_births=None, t_birth, dt0, Q=None, R=None, P0=None):
        """Start and retire tracks from an association's results on the device (target_manager_lifecycle), AFTER the tick that
        consumed the association: associate -> step_sequence_all(n_ticks=1) -> lifecycle.  det: the CUDA double tensor [M, 7] that
        was associated (None or M = 0: the retirement half alone); assoc_result: the namespace TargetManager.associate returned for
        it (its has_meas masks and slot_of_det are read; its meas / has_meas columns are stale afterwards: slots move).
        max_misses = K >= 1 retires a target on its K-th consecutive frame without a match (0: nobody).  birth_type: the motion
        model (0..3 or its name) of the targets created from the unmatched finite detections, None: no births; they get the ids
        first_id, first_id + 1, ... in ascending detection index, at most max_births of them (None: no cap), and are initialised as
        init_batch(ids, dt0, t_birth, det[j], type=birth_type, Q=Q, R=R, P0=P0) would; Q = R = P0 = None: the manager's own model
        file (birth_type must be its model).  Waits on the host.  Returns a SimpleNamespace: retired_ids (uint32 array, per batch in
        batch order, ascending former slot), born_ids (a range), retired, born, capped, non_finite."""
        from types import SimpleNamespace
        pol = capi.Lifecycle()
        pol.max_misses = int(max_misses)
        pol.birth_type = -1 if birth_type is None else _model_type(birth_type)
        pol.first_id = int(first_id)
        M = 0 if det is None else int(det.shape[0])
        pol.max_births = M if max_births is None else int(max_births)
        pol.dt0, pol.t_birth = float(dt0), float(t_birth)
        keep = []
        if birth_type is not None and not (Q is None and R is None and P0 is None):
            ns, m = MODEL_DIMS[pol.birth_type]
            for name, a, shape in (("Q", Q, (ns, ns)), ("R", R, (m, m)), ("P0", P0, (ns, ns))):
                if a is not None:
                    a = _d(a, shape)
                    keep.append(a)
                    setattr(pol, name, _dp(a))
        if det is not None:
            assert det.is_cuda and det.dim() == 2 and det.shape[1] == 7 and det.is_contiguous() and det.element_size() == 8
        masks = list(assoc_result.has_meas)
        nb = len(masks)
        mp = (C.c_void_p * max(nb, 1))()
        for i, h in enumerate(masks):
            assert h.is_cuda and h.element_size() == 1
            mp[i] = h.data_ptr()
        sod = getattr(assoc_result, "slot_of_det", None) if M > 0 else None
        if sod is not None:
            assert sod.is_cuda and sod.numel() >= M and sod.element_size() == 4, "lifecycle: slot_of_det of the device form of associate"
        cap = max(self.size(), 1)
        retired = np.empty(cap, dtype=np.uint32)
        info = (C.c_long * 6)()
        _check(self._lib.target_manager_lifecycle(self._h, None if M == 0 else det.data_ptr(), None if sod is None else sod.data_ptr(), M, mp, nb,
                                                  C.byref(pol), retired.ctypes.data_as(capi.c_uint_p), cap, info), "target_manager_lifecycle")
        return SimpleNamespace(retired_ids=retired[:info[0]].copy(), born_ids=range(info[4], info[5]), retired=info[0], born=info[1],
                               capped=info[2], non_finite=info[3])

    def find_duplicates(self, dt, gate, cell, rounds=8, min_hits=1, out=None):
        """Find pairs of tracks that follow the same object, on the device (target_manager_find_duplicates_dev; a manager on one
        device only; no host wait): the association's self-join through its grid of edge `cell`, rows with fewer than min_hits
        hits and rows whose box exceeds a cell left out.  Returns a SimpleNamespace of LISTS with one CUDA tensor per batch
        (batches() order): dup (uint8, 1 = this slot is the weaker of a matched pair), partner_batch / partner_slot (int32, -1:
        none), d2 (float64, -1: none), and info [4] = {pairs, rounds_run, settled, wide rows}.  out: such a namespace to write into."""
        import torch
        from types import SimpleNamespace
        bs = self.batches()
        nb = len(bs)
        if out is None:
            out = SimpleNamespace(dup=[torch.empty(max(b.size, 1), dtype=torch.uint8, device="cuda") for b in bs],
                                  partner_batch=[torch.empty(max(b.size, 1), dtype=torch.int32, device="cuda") for b in bs],
                                  partner_slot=[torch.empty(max(b.size, 1), dtype=torch.int32, device="cuda") for b in bs],
                                  d2=[torch.empty(max(b.size, 1), dtype=torch.float64, device="cuda") for b in bs],
                                  info=torch.empty(4, dtype=torch.int32, device="cuda"))
        per = (capi.DupOut * max(nb, 1))()
        for i in range(nb):
            per[i].dup_out_dev = out.dup[i].data_ptr()
            per[i].partner_batch_dev, per[i].partner_slot_dev = out.partner_batch[i].data_ptr(), out.partner_slot[i].data_ptr()
            per[i].d2_of_slot_dev = out.d2[i].data_ptr()
        _check(self._lib.target_manager_find_duplicates_dev(self._h, float(dt), float(gate), int(rounds), float(cell), int(min_hits), per, nb,
                                                            out.info.data_ptr()), "target_manager_find_duplicates_dev")
        return out

    def retire_duplicates(self, dt, gate, cell, rounds=8, min_hits=1):
        """Find duplicate tracks as find_duplicates does and erase the weaker track of every pair (target_manager_retire_duplicates).
        Waits on the host; slots move, so an earlier association's columns are stale afterwards.  Returns a SimpleNamespace:
        retired_ids / kept_ids (uint32 arrays, per batch in batch order, ascending former slot of the retired track), retired,
        rounds_run, settled, wide."""
        from types import SimpleNamespace
        cap = max(self.size(), 1)
        retired = np.empty(cap, dtype=np.uint32)
        kept = np.empty(cap, dtype=np.uint32)
        info = (C.c_long * 4)()
        _check(self._lib.target_manager_retire_duplicates(self._h, float(dt), float(gate), int(rounds), float(cell), int(min_hits),
                                                          retired.ctypes.data_as(capi.c_uint_p), kept.ctypes.data_as(capi.c_uint_p), cap, info),
               "target_manager_retire_duplicates")
        return SimpleNamespace(retired_ids=retired[:info[0]].copy(), kept_ids=kept[:info[0]].copy(), retired=info[0], rounds_run=info[1],
                               settled=info[2], wide=info[3])

    def get_track_counts(self, id):
        """(miss, hits) of one target as lifecycle keeps them (target_manager_get_track_counts), or None for an unknown id."""
        miss, hits = C.c_int(0), C.c_int(0)
        rc = _check(self._lib.target_manager_get_track_counts(self._h, int(id), C.byref(miss), C.byref(hits)), "target_manager_get_track_counts")
        return (miss.value, hits.value) if rc == 0 else None

    def population_tick(self):
        """True if step_sequence_all steps every batch with ONE launch per tick (target_manager_population_tick)."""
        return _check(self._lib.target_manager_population_tick(self._h), "target_manager_population_tick") == 1

    # ---- resident ("live") mode of every batch at once (target_batch_c.h)
    def live_start_all(self, dt, meas, has_meas=None, first_entry=0, max_ticks=1 << 30, idle_limit_s=10.0, query=None):
        """meas: one CUDA ring tensor [ring_ticks, 7, ld] per batch (batches() order).  query = (origin[3], radius, deltas, poses)
        adds the own-time sphere query of every target after every tick (as step_sequence_all's)."""
        nb = len(meas)
        specs = (capi.BatchSequence * max(nb, 1))()
        for i, t in enumerate(meas):
            assert t.is_cuda and t.dim() == 3 and t.shape[1] == 7 and t.stride(2) == 1
            specs[i].meas_dev, specs[i].tick_stride, specs[i].ld, specs[i].ring_ticks = t.data_ptr(), t.stride(0), t.stride(1), t.shape[0]
            if has_meas is not None and has_meas[i] is not None:
                h = has_meas[i]
                assert h.is_cuda and h.dim() == 2 and h.element_size() == 1 and h.shape[0] == t.shape[0]
                specs[i].has_meas_dev, specs[i].has_stride = h.data_ptr(), h.stride(0)
        origin, radius = None, 0.0
        if query is not None:
            origin, radius, deltas, poses = query
            origin = _d(origin, (3,))
            for i in range(nb):
                specs[i].delta_dev = deltas[i].data_ptr()
                specs[i].pose_dev = None if poses is None or poses[i] is None else poses[i].data_ptr()
        _check(self._lib.target_manager_live_start_all(self._h, float(dt), C.cast(specs, C.c_void_p), nb, int(first_entry), int(max_ticks),
                                                       float(idle_limit_s), 0 if query is None else 1, None if origin is None else _dp(origin),
                                                       float(radius)), "target_manager_live_start_all")

    def live_post_all(self, n_ticks=1, one_doorbell_per_tick=False):
        _check(self._lib.target_manager_live_post_all(self._h, int(n_ticks), 1 if one_doorbell_per_tick else 0), "target_manager_live_post_all")

    def live_done_all(self):
        return self._lib.target_manager_live_done_all(self._h)

    def live_wait_all(self, tick, timeout_s=5.0):
        return _check(self._lib.target_manager_live_wait_all(self._h, int(tick), float(timeout_s)), "target_manager_live_wait_all") == 0

    def live_stop_all(self):
        return _check(self._lib.target_manager_live_stop_all(self._h), "target_manager_live_stop_all")

    def batches(self):
        return [Batch(self._lib, self._lib.target_manager_get_batch(self._h, i))
                for i in range(self._lib.target_manager_num_batches(self._h))]

    def batch_of_type(self, type):
        h = self._lib.target_manager_get_batch_of_type(self._h, int(type))
        return Batch(self._lib, h) if h else None
