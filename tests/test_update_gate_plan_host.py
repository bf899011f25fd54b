"""CPU-only: the launch plan of an indexed request that carries the by-id update policy (csrc/step_variant.hpp, plan_step),
compiled with g++ from the product header as a stand-alone program under AddressSanitizer and UBSan: the new acceptances -- the
gated indexed kernel, with and without the fused getter table -- and every refusal that must remain."""
import os
import subprocess

from conftest import ROOT


def test_update_gate_plan(tmp_path):
    exe = str(tmp_path / "update_gate_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "update_gate_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "update gate plan host test ok" in out.stdout
