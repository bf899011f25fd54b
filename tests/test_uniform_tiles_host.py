"""CPU-only: the uniform-tile tables of the shared-axes storage form (csrc/te_layout.hpp Cfg::LIN) -- the words of a tile's block
and the record chunks a uniform tile skips, per model -- compiled with g++ from the product header."""
import os
import subprocess

from conftest import ROOT


def test_uniform_tile_tables(tmp_path):
    exe = str(tmp_path / "uniform_tiles_host_test")
    src = os.path.join(ROOT, "tests", "host", "uniform_tiles_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "uniform tiles host test ok" in out.stdout
