"""CPU-only: the launch plan of a fused request that carries the gate, the innovation stream and the policy of its call
(csrc/step_variant.hpp, plan_step), compiled with g++ from the product header as a stand-alone program under AddressSanitizer
and UBSan: the fused gated kernel is planned as kFused with StepPlan::fused_gated, the batches without it tick by tick, every
refusal holds, a request type without the member plans as it always did, and gate > 0 with n_ticks > 1 without the member still
throws."""
import os
import subprocess

from conftest import ROOT


def test_fused_gate_plan(tmp_path):
    exe = str(tmp_path / "fused_gate_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "fused_gate_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fused gate plan host test ok" in out.stdout
