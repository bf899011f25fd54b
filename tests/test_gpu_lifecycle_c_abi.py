"""tests/c_abi/lifecycle_test.c: a plain C caller (gcc -std=c99, no HIP headers) of target_manager_lifecycle and the two counter
getters behind associate_grid and one tick -- who is retired and born, with which ids and in which slots, the counters, refusals --
checked by the program itself; and examples/track_lifecycle.cpp."""
import os
import subprocess

import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def test_plain_c_caller_of_the_lifecycle(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "lifecycle_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "lifecycle_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_velocity")], capture_output=True, text=True, timeout=60)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr
    assert "lifecycle test ok" in out.stdout


def test_cpp_example_of_objects_appearing_and_vanishing(tmp_path):
    """examples/track_lifecycle.cpp: associate_grid -> one tick -> lifecycle, frame after frame"""
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "track_lifecycle")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "examples", "track_lifecycle.cpp"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, os.path.join(ROOT, "models"), "2000", "8"], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "track lifecycle example ok" in out.stdout
