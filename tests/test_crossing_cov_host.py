"""CPU-only: the HIP-free half of the crossing covariance (csrc/crossing_cov_plan.hpp) -- the predict of a chain block for NB 2 / 3
in float and double against a long double evaluation of A P A^T + Q (bound: operation count times unit round-off), its symmetry,
the filler, the refusal table, and the special cases of sigma_r / sigma_t / ok -- compiled with g++ from the product header as a
stand-alone program under AddressSanitizer and UBSan, contraction off as in the kernel."""
import os
import subprocess

from conftest import ROOT


def test_crossing_cov_plan(tmp_path):
    exe = str(tmp_path / "crossing_cov_host_test")
    src = os.path.join(ROOT, "tests", "host", "crossing_cov_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "crossing cov host test ok" in out.stdout
