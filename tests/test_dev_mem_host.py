"""CPU-only checks of the owning types of the host layer (csrc/dev_mem.hpp: device buffers, pinned blocks, streams, events) and of
the time-step table ring built on them (csrc/dt_table_ring.hpp), compiled with g++ from the product headers as a stand-alone
program under AddressSanitizer and UBSan.  The program brings malloc-backed fakes of the runtime functions the headers call and is
not linked against the HIP runtime: moves, swaps and resets release exactly once, failed allocations leave empty owners and a
clear last error, device memory only ever goes through te::device_free, a ring whose growth fails still serves, and nothing of
any kind is live at exit."""
import os
import subprocess

from conftest import ROOT

ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_dev_mem_host_program(tmp_path):
    exe = str(tmp_path / "dev_mem_host_test")
    src = os.path.join(ROOT, "tests", "host", "dev_mem_host_test.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INCLUDE, "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dev mem host test ok" in out.stdout
