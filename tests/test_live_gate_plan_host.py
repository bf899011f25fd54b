"""CPU-only: the launch plan of a resident request that carries the gate of its session (csrc/step_variant.hpp, plan_step),
compiled with g++ from the product header as a stand-alone program under AddressSanitizer and UBSan: the gated resident kernel
is planned as kFused | kLive2 with StepPlan::live_gated, every refusal holds, and a request type without the member plans as
it always did."""
import os
import subprocess

from conftest import ROOT


def test_live_gate_plan(tmp_path):
    exe = str(tmp_path / "live_gate_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "live_gate_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "live gate plan host test ok" in out.stdout
