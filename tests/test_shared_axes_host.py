"""CPU-only: the eligibility test and the record layout of the shared-axes storage form (csrc/te_layout.hpp), compiled with g++
from the product headers and run on the shipped model files."""
import os
import subprocess

from conftest import MODEL_FILES, ROOT, model_path


def test_shared_axes_eligibility_and_layout(tmp_path):
    exe = str(tmp_path / "shared_axes_host_test")
    src = os.path.join(ROOT, "tests", "host", "shared_axes_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe] + [model_path(k) for k in MODEL_FILES], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shared axes host test ok" in out.stdout
