"""CPU-only: who serves a fused replay of a whole manager (csrc/step_variant.hpp, plan_fused_all) as a table, the new launch's
predicate next to the ones it leaves alone, and the offsets of the kernel's argument struct against offsetof -- compiled with g++
from the product headers as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT


def test_fused_all_plan(tmp_path):
    exe = str(tmp_path / "fused_all_plan_host_test")
    src = os.path.join(ROOT, "tests", "host", "fused_all_plan_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fused all plan host test ok" in out.stdout
