"""The gate inside a temporally fused call at the C boundary (no GPU needed): the two symbols are exported, declared in
target_batch_c.h and bound in capi.py with the header's prototypes; NULL handles and bad gates give errors, not crashes."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = ["target_batch_step_fused_gated", "target_batch_step_fused_gate_served"]


def test_library_exports_the_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in NEW:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_calls_and_the_signatures_follow_it():
    from target_estimation_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ctype = {"long": C.c_long, "double": C.c_double, "int": C.c_int}
    pointer = {"target_pose_stream_c": C.POINTER(capi.PoseStream), "target_innov_stream_c": C.POINTER(capi.InnovStream),
               "target_reacquire_c": C.POINTER(capi.Reacquire)}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, "not declared: %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        res, sig = capi.SIGNATURES[name]
        assert res is C.c_int and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a:
                struct = [p for s, p in pointer.items() if s in a]
                assert c is (struct[0] if struct else C.c_void_p), (name, a)
            else:
                assert c is ctype[a.split()[0]], (name, a)
    # target_batch_step_fused_poses' arguments, then the stream, the gate and the policy of ..._reacquire (no ring, no use_graph)
    fused = re.search(r"\bint\s+target_batch_step_fused_poses\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    gated = re.search(r"\bint\s+target_batch_step_fused_gated\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()   # noqa: E731
    assert norm(gated) == norm(fused) + ", const target_innov_stream_c* innov, double nis_max, const target_reacquire_c* reacq"
    assert "Not served: target_batch_step_fused" not in open(HEADER).read()


def test_null_handles_give_errors():
    from target_estimation_amd import capi
    lib = capi.lib()
    assert lib.target_batch_step_fused_gate_served(None) == -1 and "NULL batch handle" in capi.last_error()
    assert lib.target_batch_step_fused_gated(None, 2, 0.004, None, 0, 0, None, 0, None, None, 0.0, None) < 0 and "NULL batch handle" in capi.last_error()
    row = (C.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    s = capi.InnovStream(C.addressof(row), None, 4, 4, 0, 0)
    assert lib.target_batch_step_fused_gated(None, 2, 0.004, None, 0, 0, None, 0, None, C.byref(s), 11.345, None) < 0
    assert "NULL batch handle" in capi.last_error()
    assert list(row) == [5.0] * 4


@pytest.mark.parametrize("nis_max,k,reason", [(-1.0, None, "nis_max"), (float("nan"), None, "nis_max"), (11.345, -1, "max_rejects"),
                                              (11.345, 128, "max_rejects"), (0.0, 3, "needs the gate")])
def test_a_bad_gate_is_refused_before_the_handle_is_looked_at(nis_max, k, reason):
    from target_estimation_amd import capi
    lib = capi.lib()
    row = (C.c_double * 4)()
    s = capi.InnovStream(C.addressof(row), None, 4, 4, 0, 0)
    r = capi.Reacquire()
    if k is not None:
        r.max_rejects = k
    assert lib.target_batch_step_fused_gated(None, 2, 0.004, None, 0, 0, None, 0, None, C.byref(s), nis_max, None if k is None else C.byref(r)) < 0
    assert reason in capi.last_error() and "NULL batch handle" not in capi.last_error(), capi.last_error()


def test_a_gate_without_rows_is_refused():
    from target_estimation_amd import capi
    lib = capi.lib()
    s = capi.InnovStream()
    assert lib.target_batch_step_fused_gated(None, 2, 0.004, None, 0, 0, None, 0, None, C.byref(s), 11.345, None) < 0 and "nis_dev" in capi.last_error()
    assert lib.target_batch_step_fused_gated(None, 2, 0.004, None, 0, 0, None, 0, None, None, 11.345, None) < 0 and "nis_dev" in capi.last_error()
