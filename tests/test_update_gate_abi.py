"""The update policy of the by-id paths at the C boundary (no GPU needed): the four symbols are exported, declared in
target_batch_c.h and bound in capi.py with the header's prototypes; NULL handles and bad policies give errors, not crashes."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = {"target_manager_set_update_gate": "int", "target_manager_get_update_gate": "int", "target_manager_update_gate_served": "int",
       "target_manager_update_meas_batch_gated": "long"}


def test_library_exports_the_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in NEW:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_calls_and_the_signatures_follow_it():
    from target_estimation_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    scalar = {"long": C.c_long, "double": C.c_double, "int": C.c_int}
    pointer = {"double": capi.c_double_p, "int": C.POINTER(C.c_int), "target_manager_c": C.c_void_p}
    for name, ret in NEW.items():
        m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (ret, name), text, flags=re.S)
        assert m, "not declared: %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        res, sig = capi.SIGNATURES[name]
        assert res is scalar[ret] and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            words = a.replace("*", " * ").split()
            if "*" in words:
                base = [w for w in words if w not in ("const", "*")]
                if base[:2] == ["unsigned", "int"]:
                    assert c is capi.c_uint_p, (name, a)
                elif base[:2] == ["unsigned", "char"]:
                    assert c is capi.c_ubyte_p, (name, a)
                else:
                    assert c is pointer[base[0]], (name, a)
            else:
                assert c is scalar[words[0]], (name, a)


def test_null_handles_give_errors():
    from target_estimation_amd import capi
    lib = capi.lib()
    g, k = C.c_double(7.0), C.c_int(7)
    assert lib.target_manager_set_update_gate(None, -1, 11.345, 3) < 0 and "NULL manager handle" in capi.last_error()
    assert lib.target_manager_get_update_gate(None, 0, C.byref(g), C.byref(k)) < 0 and (g.value, k.value) == (7.0, 7)
    assert lib.target_manager_update_gate_served(None, 0) < 0
    ids = (C.c_uint * 2)(1, 2)
    nis = (C.c_double * 2)(5.0, 5.0)
    assert lib.target_manager_update_meas_batch_gated(None, ids, 2, 0.004, None, None, nis, None) < 0
    assert list(nis) == [5.0, 5.0]


@pytest.mark.parametrize("nis_max,k", [(-1.0, -1), (float("nan"), -1), (11.345, -2), (11.345, 128), (0.0, 0), (0.0, 5)])
def test_a_bad_policy_is_refused_before_the_handle_is_looked_at(nis_max, k):
    from target_estimation_amd import capi
    lib = capi.lib()
    assert lib.target_manager_set_update_gate(None, 0, nis_max, k) < 0
    assert "update gate" in capi.last_error(), capi.last_error()
