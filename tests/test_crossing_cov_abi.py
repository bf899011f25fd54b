"""The crossing-covariance calls at the C boundary and in the Python front end (no GPU needed): the three symbols are exported,
declared in target_batch_c.h and bound in capi.py with the header's prototypes; what does not depend on a handle is refused before
the handle is looked at, and a NULL handle is an error, not a crash; manager.py hands the arguments over in the header's order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = {"target_batch_crossing_cov_dev": "int", "target_manager_crossing_cov_dev": "int", "target_manager_crossing_cov_batch": "long"}
INF, NAN = float("inf"), float("nan")


def _decl(text, name, res):
    m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (res, name), text, flags=re.S)
    assert m, "not declared: %s %s" % (res, name)
    return [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_exported_declared_and_bound():
    from target_estimation_amd import capi
    lib = capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    scalar = {"long": C.c_long, "double": C.c_double, "int": C.c_int}
    host = {"const double* origin": capi.c_double_p, "const unsigned int* ids": capi.c_uint_p, "const double* delta_host": capi.c_double_p,
            "double* cov_out": capi.c_double_p, "double* sigma_out": capi.c_double_p, "unsigned char* ok_out": capi.c_ubyte_p}
    for name, res in NEW.items():
        assert hasattr(lib, name), "not exported: %s" % name
        args = _decl(text, name, res)
        restype, sig = capi.SIGNATURES[name]
        assert restype is scalar[res] and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a:
                assert c is host.get(a, C.c_void_p), (name, a)     # host arrays typed, handles and device pointers void*
            else:
                assert c is scalar[a.split()[0]], (name, a)
    assert _decl(text, "target_batch_crossing_cov_dev", "int")[1:] == [
        "double t1", "const double* origin", "double radius", "const double* delta_dev", "const int* slots_dev", "long n",
        "double sigma_r_max", "double sigma_t_max", "double* cov_out_dev", "double* sigma_out_dev", "unsigned char* ok_out_dev"]
    whole = open(HEADER).read()
    section = whole[whole.index("POSITION COVARIANCE AND TIME SPREAD"):]
    for phrase in ("xx xy xz yy yz zz", "sigma_t", "NON-CANDIDATES", "REFUSED", "TARGET_CROSSING_COV_MAX_ROWS 8192", "Not served"):
        assert phrase in section, phrase


def test_refusals_come_before_the_handle():
    from target_estimation_amd import capi
    lib = capi.lib()
    o = (C.c_double * 3)(0.0, 0.0, 0.0)
    P = 4096          # a non-NULL pointer that is never dereferenced: every call below is refused first
    batch = lambda *a: lib.target_batch_crossing_cov_dev(None, *a)
    # (t1, origin, radius, delta, slots, n, sigma_r_max, sigma_t_max, cov, sigma, ok)
    table = [
        ((NAN, o, 1.0, None, None, 1, INF, INF, P, P, P), "delta is required"),
        ((NAN, o, 1.0, P, None, 1, INF, INF, None, P, P), "cov_out is required"),
        ((NAN, None, 1.0, P, None, 1, INF, INF, P, P, None), "sigma_out without origin"),
        ((NAN, None, 1.0, P, None, 1, INF, INF, P, None, P), "ok_out without origin"),
        ((NAN, o, 0.0, P, None, 1, INF, INF, P, P, P), "radius must be > 0"),
        ((NAN, o, -2.0, P, None, 1, INF, INF, P, None, None), "radius must be > 0"),
        ((NAN, o, NAN, P, None, 1, INF, INF, P, P, P), "radius must be > 0"),
        ((NAN, o, 1.0, P, None, 1, NAN, INF, P, P, P), "threshold is NaN"),
        ((NAN, o, 1.0, P, None, 1, INF, NAN, P, P, P), "threshold is NaN"),
        ((NAN, o, 1.0, P, None, -1, INF, INF, P, P, P), "n must be >= 0"),
        ((NAN, o, 1.0, P, P, 8193, INF, INF, P, P, P), "at most 8192"),
    ]
    for args, why in table:
        assert batch(*args) == -1, why
        err = capi.last_error()
        assert why in err and "NULL batch handle" not in err, (why, err)
    # a call with nothing to refuse reaches the handle
    assert batch(NAN, o, 1.0, P, None, 1, INF, INF, P, P, P) == -1 and "NULL batch handle" in capi.last_error()
    assert batch(NAN, None, 0.0, P, P, 8192, INF, INF, P, None, None) == -1 and "NULL batch handle" in capi.last_error()
    # the manager's forms: the same table, then the lists, then the handle
    mdev = lambda *a: lib.target_manager_crossing_cov_dev(None, *a)
    assert mdev(NAN, o, 1.0, P, P, None, 4, INF, INF, P, P, P) == -1 and "delta is required" in capi.last_error()
    assert mdev(NAN, o, 1.0, P, P, P, 8193, INF, INF, P, P, P) == -1 and "at most 8192" in capi.last_error()
    assert mdev(NAN, o, 1.0, None, P, P, 4, INF, INF, P, P, P) == -1 and "batch and slot lists" in capi.last_error()
    assert mdev(NAN, o, 1.0, P, None, P, 4, INF, INF, P, P, P) == -1 and "batch and slot lists" in capi.last_error()
    assert mdev(NAN, None, 1.0, P, P, P, 4, INF, INF, P, P, None) == -1 and "sigma_out without origin" in capi.last_error()
    assert mdev(NAN, o, 1.0, P, P, P, 4, INF, INF, P, P, P) == -1 and "NULL manager handle" in capi.last_error()
    ids = np.arange(3, dtype=np.uint32)
    d = np.zeros(3); cov = np.zeros((3, 6)); sg = np.zeros((3, 2)); ok = np.zeros(3, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)
    by_id = lambda delta, origin, radius, sr, st, c, s, k: lib.target_manager_crossing_cov_batch(
        None, ids.ctypes.data_as(capi.c_uint_p), 3, NAN, origin, radius, delta, sr, st, c, s, k)
    okp = ok.ctypes.data_as(capi.c_ubyte_p)
    assert by_id(None, o, 1.0, INF, INF, dp(cov), dp(sg), okp) == -1 and "delta is required" in capi.last_error()
    assert by_id(dp(d), o, 1.0, INF, NAN, dp(cov), dp(sg), okp) == -1 and "threshold is NaN" in capi.last_error()
    assert by_id(dp(d), None, 1.0, INF, INF, dp(cov), None, okp) == -1 and "ok_out without origin" in capi.last_error()
    assert by_id(dp(d), o, 1.0, INF, INF, dp(cov), dp(sg), okp) == -1 and "NULL manager handle" in capi.last_error()
    assert not cov.any() and not sg.any() and not ok.any(), "a refused call wrote to its outputs"


class _Lib:
    """a library stub: records every call, returns 0"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Tensor:
    """what manager.py reads of a CUDA tensor"""
    def __init__(self, n, addr):
        self.shape, self._addr = (n,), addr

    def data_ptr(self):
        return self._addr


def test_the_front_end_hands_the_arguments_over_in_the_headers_order():
    pytest.importorskip("torch")
    from target_estimation_amd import manager
    lib = _Lib()
    b = manager.Batch(lib, 7)
    delta, slots, cov = _Tensor(5, 1000), _Tensor(5, 2000), _Tensor(5, 3000)
    b.crossing_cov(delta, slots, sigma_r_max=0.25, out=(cov, None, None))
    name, a = lib.calls[-1]
    assert name == "target_batch_crossing_cov_dev"
    assert a[0] == 7 and np.isnan(a[1]) and a[2] is None and a[4:8] == (1000, 2000, 5, 0.25) and a[8] == INF and a[9:] == (3000, None, None)
    sg, ok = _Tensor(5, 4000), _Tensor(5, 5000)
    b.crossing_cov(delta, None, origin=[1.0, 2.0, 3.0], radius=1.5, t1=0.048, sigma_t_max=0.002, out=(cov, sg, ok))
    name, a = lib.calls[-1]
    assert a[1] == 0.048 and [a[2][i] for i in range(3)] == [1.0, 2.0, 3.0] and a[3] == 1.5
    assert a[4:] == (1000, None, 5, INF, 0.002, 3000, 4000, 5000)
