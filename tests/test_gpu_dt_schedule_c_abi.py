"""tests/c_abi/dt_schedule_test.c: a plain C caller (gcc -std=c99, no HIP headers) of the calls with a time step per tick in
target_batch_c.h -- it steps one stream through target_batch_step_sequence_dt, target_batch_step_fused_dt and
target_manager_step_sequence_all_dt and compares every byte with single target_batch_step calls through the same ABI -- on a GPU."""
import os
import subprocess

import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def test_plain_c_caller_of_the_schedule_calls(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "dt_schedule_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "dt_schedule_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_acceleration")], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dt schedule test ok" in out.stdout
