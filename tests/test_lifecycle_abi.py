"""The track lifecycle at the C boundary and in the Python front end (no GPU needed): the three symbols are exported, declared in
target_batch_c.h and bound in capi.py with the header's prototypes; the header carries the contract; what does not depend on a handle is
refused before the handle is looked at, and a NULL handle is an error, not a crash."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = {"target_manager_lifecycle": "int", "target_batch_track_counts": "int", "target_manager_get_track_counts": "int"}
NAN = float("nan")


def _decl(text, name, res):
    m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (res, name), text, flags=re.S)
    assert m, "not declared: %s %s" % (res, name)
    return [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_exported_declared_and_bound():
    from target_estimation_amd import capi
    lib = capi.lib()
    whole = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    scalar = {"long": C.c_long, "double": C.c_double, "int": C.c_int, "unsigned int": C.c_uint}
    host = {"const unsigned char* const* has_meas_dev": C.POINTER(C.c_void_p), "const target_lifecycle_c* policy": C.POINTER(capi.Lifecycle),
            "unsigned int* retired_ids_out": capi.c_uint_p, "long* info": C.POINTER(C.c_long), "unsigned char* miss_host": capi.c_ubyte_p,
            "unsigned char* hits_host": capi.c_ubyte_p, "int* miss": C.POINTER(C.c_int), "int* hits": C.POINTER(C.c_int)}
    for name, res in NEW.items():
        assert hasattr(lib, name), "not exported: %s" % name
        args = _decl(text, name, res)
        restype, sig = capi.SIGNATURES[name]
        assert restype is scalar[res] and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a:
                assert c is host.get(a, C.c_void_p), (name, a)
            else:
                assert c is scalar[a.rsplit(" ", 1)[0]], (name, a)
    assert _decl(text, "target_manager_lifecycle", "int") == [
        "target_manager_c* m", "const double* det_dev", "const int* slot_of_det_dev", "long M", "const unsigned char* const* has_meas_dev",
        "long n_batches", "const target_lifecycle_c* policy", "unsigned int* retired_ids_out", "long retired_cap", "long* info"]
    # the struct: the header's fields, in order, are the ctypes struct's
    m = re.search(r"typedef struct target_lifecycle_c \{(.*?)\} target_lifecycle_c;", text, flags=re.S)
    fields = [f.strip().rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    ctype = {"int": C.c_int, "unsigned int": C.c_uint, "long": C.c_long, "double": C.c_double, "const double*": capi.c_double_p}
    assert [(n, ctype[t]) for t, n in fields] == list(capi.Lifecycle._fields_)


def test_header_carries_the_contract():
    whole = open(HEADER).read()
    section = whole[whole.index("TRACK LIFECYCLE"):whole.index("typedef struct target_lifecycle_c")]
    section = re.sub(r"\s*\n \*\s*", " ", section)   # (the comment's line breaks are not part of the contract)
    for phrase in ("associate -> step -> lifecycle", "STALE afterwards", "left untouched", "saturates at 255", "0 at creation",
                   "only lifecycle calls write them", "function of the inputs alone", "max_misses = 0 retires nobody",
                   "the lowest detection indices win", "ascending former slot", "bit for bit", "NOTHING CHANGES on a refusal",
                   "TARGET_ASSOC_GRID_MAX_DETECTIONS", "wrapping past 2^32 - 1", "before the handle is looked at", "WAITS ON THE HOST",
                   "NOT CAPTURABLE", "recorded sequences, uniform tiles, shared-axes batches and live sessions",
                   "Queued one-target steps and inits run first", "Not built", "merging several unmatched detections", "time-based (seconds) expiry",
                   "confirmed-only mask", "several shards", "the Eigen facade", "(M = 0)"):
        assert phrase in section, phrase


def test_python_signatures():
    import target_estimation_amd as te
    p = inspect.signature(te.TargetManager.lifecycle).parameters
    assert list(p)[:3] == ["self", "det", "assoc_result"]
    kw = ["max_misses", "birth_type", "first_id", "max_births", "t_birth", "dt0", "Q", "R", "P0"]
    assert list(p)[3:] == kw and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    for k in ("birth_type", "max_births", "Q", "R", "P0"):
        assert p[k].default is None
    for k in ("max_misses", "first_id", "t_birth", "dt0"):
        assert p[k].default is inspect.Parameter.empty
    assert list(inspect.signature(te.Batch.track_counts).parameters) == ["self"]


def _policy(capi, **kw):
    p = capi.Lifecycle()
    p.max_misses, p.birth_type, p.first_id, p.max_births, p.dt0, p.t_birth = 3, 3, 100, 16, 0.01, 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_refusals_come_before_the_handle_and_null_handles_are_errors():
    from target_estimation_amd import capi
    lib = capi.lib()
    P = 4096          # a non-NULL pointer that is never dereferenced: every call below is refused first
    masks = (C.c_void_p * 2)(P, P)
    retired = (C.c_uint * 4)()
    info = (C.c_long * 6)()
    one = (C.c_double * 1)(1.0)
    dp = C.cast(one, capi.c_double_p)
    big = (1 << 20) + 1
    # (det, slot_of_det, M, masks, n_batches, policy, retired, retired_cap, info)
    good = [P, P, 8, masks, 2, C.byref(_policy(capi)), retired, 4, info]
    table = [({5: None}, "policy is required"), ({8: None}, "info is required"), ({2: -1}, "M must be 0..1048576"), ({2: big}, "M must be 0..1048576"),
             ({5: C.byref(_policy(capi, max_misses=-1))}, "max_misses must be 0..255"), ({5: C.byref(_policy(capi, max_misses=256))}, "max_misses must be 0..255"),
             ({5: C.byref(_policy(capi, birth_type=-2))}, "birth_type must be -1..3"), ({5: C.byref(_policy(capi, birth_type=4))}, "birth_type must be -1..3"),
             ({5: C.byref(_policy(capi, max_births=-1))}, "max_births must be >= 0"),
             ({5: C.byref(_policy(capi, t_birth=NAN))}, "must not be NaN"), ({5: C.byref(_policy(capi, dt0=NAN))}, "must not be NaN"),
             ({5: C.byref(_policy(capi, Q=dp))}, "together or not at all"), ({5: C.byref(_policy(capi, Q=dp, R=dp))}, "together or not at all"),
             ({5: C.byref(_policy(capi, P0=dp))}, "together or not at all"),
             ({0: None}, "required for births"), ({1: None}, "required for births"),
             ({4: -1}, "one mask per batch"), ({3: None}, "one mask per batch"),
             ({7: -1}, "retired_ids_out"), ({6: None}, "retired_ids_out"),
             ({2: 1 << 20}, "NULL manager handle"), ({}, "NULL manager handle"),
             ({0: None, 1: None, 5: C.byref(_policy(capi, birth_type=-1))}, "NULL manager handle"),      # the retirement half needs no frame
             ({0: None, 1: None, 2: 0}, "NULL manager handle"),
             ({5: C.byref(_policy(capi, Q=dp, R=dp, P0=dp))}, "NULL manager handle")]
    for change, why in table:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.target_manager_lifecycle(None, *args) == -1, why
        assert why in capi.last_error() and "target_manager_lifecycle" in capi.last_error(), (why, capi.last_error())
    # the getters
    b = (C.c_ubyte * 4)()
    assert lib.target_batch_track_counts(None, b, b) == -1 and "NULL batch handle" in capi.last_error()
    i = C.c_int(0)
    assert lib.target_manager_get_track_counts(None, 1, C.byref(i), C.byref(i)) == -1 and "NULL manager handle" in capi.last_error()
    assert lib.target_manager_get_track_counts(None, 1, None, C.byref(i)) == -1 and "must not be NULL" in capi.last_error()
