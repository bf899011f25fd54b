"""tests/c_abi/find_duplicates_test.c: a plain C caller (gcc -std=c99, no HIP headers) of target_manager_find_duplicates_dev and
target_manager_retire_duplicates -- who is the duplicate of whom, ids, slots and counters afterwards, refusals -- checked by the
program itself; and examples/duplicate_tracks.cpp."""
import os
import subprocess

import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def test_plain_c_caller_of_the_duplicate_search(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "find_duplicates_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "find_duplicates_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_velocity")], capture_output=True, text=True, timeout=60)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr
    assert "find duplicates test ok" in out.stdout


def test_cpp_example_of_a_detector_that_splits_objects(tmp_path):
    """examples/duplicate_tracks.cpp: the population with and without target_manager_retire_duplicates"""
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "duplicate_tracks")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "examples", "duplicate_tracks.cpp"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, os.path.join(ROOT, "models"), "2000", "8"], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "duplicate tracks example ok" in out.stdout
