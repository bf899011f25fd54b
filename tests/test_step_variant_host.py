"""CPU-only: the step kernels' variant word and the launch plan of OpsImpl::step (csrc/step_variant.hpp), compiled with g++ from
the product header: every request against every kind of OpsImpl, and the launch sequence of every request the library serves,
row by row.  And the tools' table of the variant's names (tools/step_variant.py) against the bits of the header."""
import os
import re
import subprocess
import sys

from conftest import ROOT


def test_step_variant_plan(tmp_path):
    exe = str(tmp_path / "step_variant_host_test")
    src = os.path.join(ROOT, "tests", "host", "step_variant_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step variant host test ok" in out.stdout


def test_tools_table_equals_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import step_variant as sv
    finally:
        sys.path.pop(0)
    hdr = open(os.path.join(ROOT, "target_estimation_amd", "csrc", "step_variant.hpp")).read()
    enum = re.search(r"enum StepVariantBit : unsigned \{(.*?)\};", hdr, re.S).group(1)
    bits = {m.group(1).upper(): int(m.group(2)) << int(m.group(3)) for m in re.finditer(r"\bk(\w+) = (\d+)u << (\d+)", enum)}
    assert len(bits) == 9, bits
    live = {n: bits.pop(n) for n in ("LIVE1", "LIVE2")}
    assert bits == sv.BITS
    assert live == {"LIVE1": 1 << sv.LIVE_SHIFT, "LIVE2": 2 << sv.LIVE_SHIFT}
    assert sv.variant_name(bits["FUSED"] | live["LIVE2"]) == "FUSED|LIVE2" and sv.variant_word("FUSED", "LIVE2") == bits["FUSED"] | live["LIVE2"]
    assert sv.variant_name(0) == "0" and sv.variant_word() == 0
    for v in range(1 << 9):
        if (v >> sv.LIVE_SHIFT) & 3 != 3:
            assert sv.variant_word(*sv.variant_name(v).split("|")) == v if v else True
    assert sv.name_variants("te::kf_step_kernel<te::ModelAR, float, 3, 0, 24u>") == "te::kf_step_kernel<te::ModelAR, float, 3, 0, PERQR|AB>"
    assert sv.name_variants("te::outputs_kernel<te::ModelAR, float, 3, 0>") == "te::outputs_kernel<te::ModelAR, float, 3, 0>"
