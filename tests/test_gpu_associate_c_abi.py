"""tests/c_abi/associate_test.c: a plain C caller (gcc -std=c99, no HIP headers) of the four association symbols on a two-model
manager -- the pairing of a reversed frame with clutter, the scattered measurements feeding target_batch_step, ids and the unmatched
list of the host forms, refusals -- checked by the program itself; and examples/associate_detections.cpp."""
import os
import subprocess

import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def test_plain_c_caller_of_the_association(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "associate_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "associate_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_acceleration")], capture_output=True, text=True, timeout=60)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr
    assert "associate test ok" in out.stdout


def test_cpp_example_of_a_shuffled_frame(tmp_path):
    """examples/associate_detections.cpp: a shuffled frame in, associate, one gated tick"""
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "associate_detections")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "examples", "associate_detections.cpp"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, os.path.join(ROOT, "models"), "2000", "5"], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "associate detections example ok" in out.stdout
