"""The per-tick innovation / NIS stream of launched ticks at the C boundary, and the achievability of the GPU tests' bound (no GPU
needed): the two ..._innov symbols are exported and bound, the header declares target_innov_stream_c with its fields in order, the
ctypes mirror has the header's size and field offsets (taken from a C compiler reading the header itself), and an independent
implementation -- the CPU oracle in f64 and in f32, its innovations formed in numpy -- stays inside the bound of
tests/innov_stream_ref.py against the np_twin reference."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import HARNESS_ORDER, ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
INNOV_SYMBOLS = ["target_batch_step_sequence_innov", "target_manager_step_sequence_all_innov"]
FIELDS = ["nis_dev", "innov_dev", "ld", "nis_tick_stride", "innov_tick_stride", "ring_ticks"]


def test_library_exports_the_innovation_stream_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in INNOV_SYMBOLS:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_innovation_stream():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+target_innov_stream_c\s*\{(.*?)\}\s*target_innov_stream_c\s*;", text, flags=re.S)
    assert m, "target_batch_c.h does not declare target_innov_stream_c"
    body = m.group(1)
    assert re.findall(r"(\w+)\s*;", body) == FIELDS
    assert re.search(r"double\s*\*\s*nis_dev\s*;", body) and re.search(r"double\s*\*\s*innov_dev\s*;", body)
    for name in INNOV_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), "not declared: %s" % name
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).replace(" *", "*")
        assert "target_innov_stream_c*" in args and "target_pose_stream_c*" in args


def test_ctypes_mirror_matches_the_header_layout(tmp_path):
    from target_estimation_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "target_batch_c.h"\n'
                   "int main(void) { printf(\"%s\\n\", sizeof(target_innov_stream_c), %s); return 0; }\n"
                   % (" ".join(["%zu"] * (len(FIELDS) + 1)), ", ".join("offsetof(target_innov_stream_c, %s)" % f for f in FIELDS)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    size, *offsets = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert size == 48
    assert ctypes.sizeof(capi.InnovStream) == size
    assert [f[0] for f in capi.InnovStream._fields_] == FIELDS
    assert [getattr(capi.InnovStream, f).offset for f in FIELDS] == offsets


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", HARNESS_ORDER)
def test_the_bound_is_achievable_by_an_independent_implementation(models, name, dtype):
    """The oracle (f64 and f32) over the GPU tests' own stream -- 20 ticks, masks, the predict-only run; 24 targets here -- with nu
    and NIS formed in numpy at that precision from its state before each tick: inside the bound against the twin, every target,
    every tick."""
    import innov_stream_ref as ref
    m = models[name]
    p0, meas, mask, want = ref.stream_and_reference(name, 24, 20, 31)
    nu, nis = ref.oracle_innovations(m["model"], m["Q"], m["R"], m["P"], p0, meas, mask, 0.004, dtype)
    ref.check(nu, nis, want, mask, dtype, "%s %s oracle" % (name, dtype))
