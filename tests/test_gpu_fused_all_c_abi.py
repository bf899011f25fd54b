"""tests/c_abi/fused_all_test.c: a plain C caller (gcc -std=c99, no HIP headers) of the manager-level fused replay in
target_batch_c.h -- it makes the manager-level calls on a two-model manager and compares every row with the per-batch fused calls
through the same ABI -- on a GPU."""
import os
import subprocess

import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def test_plain_c_caller_of_the_fused_replay_of_a_manager(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "fused_all_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "fused_all_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_acceleration")], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fused all test ok" in out.stdout
