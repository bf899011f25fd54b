"""The per-tick pose stream of launched ticks at the C boundary (no GPU needed): the three ..._poses symbols are exported and
bound, the header declares target_pose_stream_c, and the ctypes mirror has the header's size and field offsets (taken from a C
compiler reading the header itself)."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
POSE_SYMBOLS = ["target_batch_step_sequence_poses", "target_batch_step_fused_poses", "target_manager_step_sequence_all_poses"]
FIELDS = ["pose_dev", "ld", "tick_stride", "ring_ticks"]


def test_library_exports_the_pose_stream_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    for name in POSE_SYMBOLS:
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not bound in capi.SIGNATURES: %s" % name


def test_header_declares_the_pose_stream():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+target_pose_stream_c\s*\{(.*?)\}\s*target_pose_stream_c\s*;", text, flags=re.S)
    assert m, "target_batch_c.h does not declare target_pose_stream_c"
    body = m.group(1)
    assert re.findall(r"(\w+)\s*;", body) == FIELDS
    assert re.search(r"double\s*\*\s*pose_dev\s*;", body)
    for name in POSE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), "not declared: %s" % name
        assert "target_pose_stream_c*" in re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).replace(" *", "*")


def test_ctypes_mirror_matches_the_header_layout(tmp_path):
    from target_estimation_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "target_batch_c.h"\n'
                   "int main(void) { printf(\"%%zu %%zu %%zu %%zu %%zu\\n\", sizeof(target_pose_stream_c), %s); return 0; }\n"
                   % ", ".join("offsetof(target_pose_stream_c, %s)" % f for f in FIELDS))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    size, *offsets = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert size == 32
    assert ctypes.sizeof(capi.PoseStream) == size
    assert [f[0] for f in capi.PoseStream._fields_] == FIELDS
    assert [getattr(capi.PoseStream, f).offset for f in FIELDS] == offsets
