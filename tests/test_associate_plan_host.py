"""CPU-only: the HIP-free half of the association of unlabelled detections (csrc/associate_plan.hpp) -- the refusal table, the grid
plan's exact cover for awkward sizes and forced chunk counts, the tie rule of a partial minimum and of the merge, the inverse of S
and its validity rule, d^2 -- compiled with g++ from the product header as a stand-alone program under AddressSanitizer and UBSan,
contraction off as in the kernels."""
import os
import subprocess

from conftest import ROOT


def test_associate_plan(tmp_path):
    exe = str(tmp_path / "associate_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "associate_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "associate plan host test ok" in out.stdout
