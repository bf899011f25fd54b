"""CPU-only: the HIP-free half of the track lifecycle (csrc/lifecycle_plan.hpp) -- the refusal table, the counters with their
saturation, the stale and finiteness rules, the block cover for awkward sizes, the ordered compaction's block arithmetic against a
sequential pass, the id-range wrap check -- compiled with g++ from the product header as a stand-alone program under
AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT


def test_lifecycle_plan(tmp_path):
    exe = str(tmp_path / "lifecycle_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "lifecycle_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lifecycle plan host test ok" in out.stdout
