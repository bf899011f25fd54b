"""The NIS validation gate at the C boundary (no GPU needed): the two ..._gated symbols are exported, declared and bound, their
ctypes signatures are the header's, and a bad nis_max -- negative, NaN, or positive without a NIS row -- is refused with a message
that names the gate before a handle or a device is looked at."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
GATED = ["target_batch_step_sequence_gated", "target_manager_step_sequence_all_gated"]


def test_library_exports_the_gated_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in GATED:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_gated_calls_and_the_signatures_follow_it():
    from target_estimation_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ctype = {"long": C.c_long, "double": C.c_double, "int": C.c_int}
    for name in GATED:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, "not declared: %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        assert any(re.match(r"(const\s+)?double\s*\*?\s*(per_batch_)?nis_max$", a) for a in args), args
        assert args[-1] == "int use_graph"
        res, sig = capi.SIGNATURES[name]
        assert res is C.c_int and len(sig) == len(args)
        for a, c in zip(args, sig):
            if "*" in a:
                assert c not in (C.c_long, C.c_double, C.c_int), (name, a)
            else:
                assert c is ctype[a.split()[0]], (name, a)
    full = open(HEADER).read()
    assert "11.345" in full and "16.812" in full


@pytest.mark.parametrize("nis_max", [-1.0, float("nan"), -float("inf"), 11.345])
def test_bad_nis_max_is_refused_before_anything_else(nis_max):
    """(11.345 without a stream: the gate's decisions are reported through the NIS row)"""
    from target_estimation_amd import capi
    lib = capi.lib()
    rc = lib.target_batch_step_sequence_gated(None, 1, 0.004, None, 0, 0, None, 0, 0, None, None, nis_max, 0)
    assert rc < 0 and "gate" in capi.last_error(), capi.last_error()
    gates = (C.c_double * 2)(0.0, nis_max)
    rc = lib.target_manager_step_sequence_all_gated(None, 1, 0.004, None, None, None, gates, 2, 0, None, 0.0, 0)
    assert rc < 0 and "gate" in capi.last_error(), capi.last_error()
    no_row = (capi.InnovStream * 2)()   # (streams without a NIS row)
    rc = lib.target_manager_step_sequence_all_gated(None, 1, 0.004, None, None, no_row, gates, 2, 0, None, 0.0, 0)
    assert rc < 0 and "gate" in capi.last_error(), capi.last_error()
