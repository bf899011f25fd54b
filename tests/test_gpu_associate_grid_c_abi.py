"""tests/c_abi/associate_grid_test.c: a plain C caller (gcc -std=c99, no HIP headers) of the four grid-form association symbols on a
two-model manager -- the pairing of a reversed frame with clutter against the brute-force sibling's, the wide count at both extremes
of cell, the scattered measurements feeding target_batch_step, ids and the unmatched list of the host forms, refusals -- checked by
the program itself."""
import os
import subprocess

import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def test_plain_c_caller_of_the_grid_association(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "associate_grid_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "associate_grid_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_acceleration")], capture_output=True, text=True, timeout=60)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr
    assert "associate grid test ok" in out.stdout
