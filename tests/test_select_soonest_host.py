"""CPU-only: the HIP-free half of the k-soonest selection (csrc/select_soonest_plan.hpp) -- the key order with +-0, ties and the
filler, the argument checks as a table, the split of the first stage's grid, and the merge of the shards' rows against a
brute-force sort -- compiled with g++ from the product header as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT


def test_select_soonest_plan(tmp_path):
    exe = str(tmp_path / "select_soonest_host_test")
    src = os.path.join(ROOT, "tests", "host", "select_soonest_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "select soonest host test ok" in out.stdout
