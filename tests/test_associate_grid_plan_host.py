"""CPU-only: the HIP-free half of the grid form of the association (csrc/associate_grid_plan.hpp) -- the refusal table, the
bucket-count plan with forced values, the neighbour property of the cell map on random and adversarial inputs, the box rule, the
keyed pick against a sorted pass -- compiled with g++ from the product header as a stand-alone program under AddressSanitizer and
UBSan, contraction off as in the kernels."""
import os
import subprocess

from conftest import ROOT


def test_associate_grid_plan(tmp_path):
    exe = str(tmp_path / "associate_grid_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "associate_grid_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "associate grid plan host test ok" in out.stdout
