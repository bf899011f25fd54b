"""CPU-only: the host logic of the re-acquisition (csrc/step_variant.hpp plan_step with the request field reacq;
csrc/reacquire_plan.hpp: the policy's checks and the bookkeeping of the device tables through append, single erase and batched
erase), compiled with g++ from the product headers as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT


def test_reacquire_plan(tmp_path):
    exe = str(tmp_path / "reacquire_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "reacquire_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reacquire plan host test ok" in out.stdout
