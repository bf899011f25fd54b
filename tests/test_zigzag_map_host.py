"""CPU-only: the block order of a reversed dense tick (csrc/zigzag_map.hpp zz_block), compiled with g++ from the product header:
a bijection of [0, n) that is its own inverse, keeps b % 8 and walks every class from its last block down, for n = 1 .. 300."""
import os
import subprocess

from conftest import ROOT


def test_zigzag_map(tmp_path):
    exe = str(tmp_path / "zigzag_map_host_test")
    src = os.path.join(ROOT, "tests", "host", "zigzag_map_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "zigzag map host test ok" in out.stdout
