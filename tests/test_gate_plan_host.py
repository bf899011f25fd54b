"""CPU-only: the launch plan of a request with a validation gate (csrc/step_variant.hpp, plan_step), compiled with g++ from the
product header as a stand-alone program under AddressSanitizer and UBSan: the gated kInnov kernel for one-class separable batches,
the writer's mask row and the plain step for everything else, the refusals, and a request type without the gate member, which
plans as before."""
import os
import subprocess

from conftest import ROOT


def test_gate_plan(tmp_path):
    exe = str(tmp_path / "gate_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "gate_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gate plan host test ok" in out.stdout
