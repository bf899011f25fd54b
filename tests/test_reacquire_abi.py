"""The re-acquisition calls at the C boundary (no GPU needed): the four symbols are exported, declared and bound, their ctypes
signatures and the struct are the header's, and a bad policy -- K outside 0..127, a policy without a gate, malformed event rows
-- is refused with a message that names the re-acquisition before a handle or a device is looked at."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = ["target_batch_step_sequence_reacquire", "target_manager_step_sequence_all_reacquire", "target_batch_rejection_runs",
       "target_manager_get_rejection_run"]


def test_library_exports_the_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in NEW:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_calls_and_the_signatures_follow_it():
    from target_estimation_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ctype = {"long": C.c_long, "double": C.c_double, "int": C.c_int, "unsigned": C.c_uint}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, "not declared: %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        res, sig = capi.SIGNATURES[name]
        assert res is C.c_int and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a:
                assert c not in (C.c_long, C.c_double, C.c_int, C.c_uint), (name, a)
            else:
                assert c is ctype[a.split()[0]], (name, a)
    for name in NEW[:2]:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert re.search(r"const\s+target_reacquire_c\s*\*\s*(per_batch_)?reacq\b", args) and args.strip().endswith("int use_graph")
    m = re.search(r"typedef\s+struct\s+target_reacquire_c\s*\{(.*?)\}\s*target_reacquire_c\s*;", text, flags=re.S)
    assert m, "target_reacquire_c is not declared"
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert [f.split()[-1].lstrip("*") for f in fields] == [n for n, _ in capi.Reacquire._fields_]
    assert [t for _, t in capi.Reacquire._fields_] == [C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_long]


@pytest.mark.parametrize("k,gate,ld,stride,ring", [(-1, 300.0, 8, 8, 0), (128, 300.0, 8, 8, 0), (3, 0.0, 8, 8, 0), (3, 300.0, 8, 4, 0),
                                                   (3, 300.0, 8, -8, 0), (3, 300.0, 8, 8, -1), (3, 300.0, 0, 0, 0)])
def test_a_bad_policy_is_refused_before_anything_else(k, gate, ld, stride, ring):
    from target_estimation_amd import capi
    lib = capi.lib()
    row = (C.c_ubyte * 64)()
    nis = (C.c_double * 8)()    # (never dereferenced: the call is refused before a handle is looked at)
    stream = capi.InnovStream(C.addressof(nis), None, 8, 8, 0, 0)
    policy = capi.Reacquire(k, C.addressof(row), ld, stride, ring)
    rc = lib.target_batch_step_sequence_reacquire(None, 1, 0.004, None, 0, 0, None, 0, 0, None, C.byref(stream), gate, C.byref(policy), 0)
    assert rc < 0 and "re-acquisition" in capi.last_error(), capi.last_error()
    if k >= 0:   # (in a per-batch array a negative max_rejects means: no policy for that batch)
        streams = (capi.InnovStream * 2)(stream, stream)
        gates = (C.c_double * 2)(300.0, gate)
        policies = (capi.Reacquire * 2)(capi.Reacquire(0, None, 0, 0, 0), policy)
        rc = lib.target_manager_step_sequence_all_reacquire(None, 1, 0.004, None, None, streams, gates, policies, 2, 0, None, 0.0, 0)
        assert rc < 0 and "re-acquisition" in capi.last_error(), capi.last_error()


def test_the_getters_refuse_null_handles():
    from target_estimation_amd import capi
    lib = capi.lib()
    assert lib.target_batch_rejection_runs(None, None) < 0
    assert lib.target_manager_get_rejection_run(None, 3) < 0
