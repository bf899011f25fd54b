"""The gate of the resident sessions at the C boundary (no GPU needed): the two symbols are exported, declared in
target_batch_c.h and bound in capi.py with the header's prototypes; NULL handles and bad gates give errors, not crashes."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = {"target_batch_live_set_gate": "int", "target_batch_live_gate_served": "int"}


def test_library_exports_the_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in NEW:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_calls_and_the_signatures_follow_it():
    from target_estimation_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    scalar = {"double": C.c_double, "int": C.c_int}
    for name, ret in NEW.items():
        m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), text, flags=re.S)
        assert m, "not declared: %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        res, sig = capi.SIGNATURES[name]
        assert res is scalar[ret] and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a:   # handles and structs travel as untyped pointers (capi.InnovStream / capi.Reacquire by reference)
                assert c is C.c_void_p, (name, a)
            else:
                assert c is scalar[a.split()[0]], (name, a)
    # the structs the call reuses are the launched calls' own
    assert re.search(r"target_batch_live_set_gate\s*\([^)]*const\s+struct\s+target_innov_stream_c\s*\*[^)]*const\s+struct\s+target_reacquire_c\s*\*", text)


def test_null_handles_give_errors():
    from target_estimation_amd import capi
    lib = capi.lib()
    assert lib.target_batch_live_gate_served(None) == -1 and "NULL batch handle" in capi.last_error()
    assert lib.target_batch_live_set_gate(None, 0.0, None, None) < 0 and "NULL batch handle" in capi.last_error()
    s = capi.InnovStream()
    row = (C.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    s.nis_dev, s.ld = C.addressof(row), 4
    assert lib.target_batch_live_set_gate(None, 11.345, C.byref(s), None) < 0 and "NULL batch handle" in capi.last_error()
    assert list(row) == [5.0] * 4


@pytest.mark.parametrize("nis_max,k,reason", [(-1.0, None, "nis_max"), (float("nan"), None, "nis_max"), (11.345, -1, "max_rejects"),
                                              (11.345, 128, "max_rejects"), (0.0, 3, "needs the gate")])
def test_a_bad_gate_is_refused_before_the_handle_is_looked_at(nis_max, k, reason):
    from target_estimation_amd import capi
    lib = capi.lib()
    s = capi.InnovStream()
    row = (C.c_double * 4)()
    s.nis_dev, s.ld = C.addressof(row), 4
    r = capi.Reacquire()
    if k is not None:
        r.max_rejects = k
    assert lib.target_batch_live_set_gate(None, nis_max, C.byref(s), None if k is None else C.byref(r)) < 0
    assert reason in capi.last_error(), capi.last_error()


def test_a_gate_without_rows_or_with_an_innovation_block_is_refused():
    from target_estimation_amd import capi
    lib = capi.lib()
    s = capi.InnovStream()
    assert lib.target_batch_live_set_gate(None, 11.345, C.byref(s), None) < 0 and "nis_dev" in capi.last_error()
    row = (C.c_double * 4)()
    s.nis_dev, s.innov_dev, s.ld = C.addressof(row), C.addressof(row), 4
    assert lib.target_batch_live_set_gate(None, 11.345, C.byref(s), None) < 0 and "innov_dev" in capi.last_error()
