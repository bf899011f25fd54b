"""CPU-only: the HIP-free half of the duplicate-track search (csrc/track_merge_plan.hpp) -- the refusal table, the claim that a
pair's box never exceeds the larger of its two rows' boxes (random and adversarial Sigma), the neighbour property for narrow pairs
on cell borders and at the clamp, d2 symmetry under the (lo, hi) order, the keyed pick under shuffled visiting orders with repeats,
the survivor rule -- compiled with g++ from the product header as a stand-alone program under AddressSanitizer and UBSan,
contraction off as in the kernels."""
import os
import subprocess

from conftest import ROOT


def test_track_merge_plan(tmp_path):
    exe = str(tmp_path / "track_merge_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "track_merge_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "track merge plan host test ok" in out.stdout
