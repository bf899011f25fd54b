"""The manager-level fused replay at the C boundary (no GPU needed): the three symbols are exported, declared in target_batch_c.h
and bound in capi.py with the header's prototypes; NULL handles give errors with last_error set, not crashes."""
import ctypes as C
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = ["target_manager_step_fused_all", "target_manager_step_fused_all_dt", "target_manager_step_fused_all_served"]


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
               "target_reacquire_c": C.POINTER(capi.Reacquire), "double*": capi.c_double_p}
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
    # the scalar call's arguments with dt_host in place of dt
    norm = lambda s: re.sub(r"\s+", " ", s).strip()   # noqa: E731
    one = norm(re.search(r"\bint\s+target_manager_step_fused_all\s*\((.*?)\)\s*;", text, flags=re.S).group(1))
    sched = norm(re.search(r"\bint\s+target_manager_step_fused_all_dt\s*\((.*?)\)\s*;", text, flags=re.S).group(1))
    assert sched == one.replace("double dt,", "const double* dt_host,")
    assert "Not served: a manager-level fused call" not in open(HEADER).read()


def test_null_handles_give_errors():
    from target_estimation_amd import capi
    lib = capi.lib()
    assert lib.target_manager_step_fused_all_served(None, 0, 0) == -1 and "NULL manager handle" in capi.last_error()
    assert lib.target_manager_step_fused_all_served(None, 1, 1) == -1 and "NULL manager handle" in capi.last_error()
    specs = (capi.BatchSequence * 2)()
    assert lib.target_manager_step_fused_all(None, 2, 0.004, C.cast(specs, C.c_void_p), None, None, None, None, 2) < 0
    assert "NULL manager handle" in capi.last_error()
    dts = (C.c_double * 2)(0.004, 0.004)
    assert lib.target_manager_step_fused_all_dt(None, 2, dts, C.cast(specs, C.c_void_p), None, None, None, None, 2) < 0
    assert "NULL manager handle" in capi.last_error()
    assert lib.target_manager_step_fused_all_dt(None, 2, None, None, None, None, None, None, 0) < 0 and capi.last_error()
