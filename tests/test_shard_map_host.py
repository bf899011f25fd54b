"""CPU-only checks of the id -> shard map and placement rule of a manager spread over several devices (csrc/shard_map.hpp),
compiled with g++ and the sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_shard_placement_merge_and_ranks(tmp_path):
    exe = str(tmp_path / "shard_map_test")
    src = os.path.join(ROOT, "tests", "host", "shard_map_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shard map tests ok" in out.stdout
