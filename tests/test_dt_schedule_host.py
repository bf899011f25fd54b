"""CPU-only checks of the time-step schedule's host side, compiled with g++ from the product headers as stand-alone programs under
AddressSanitizer and UBSan: csrc/dt_schedule.hpp (the clock over a schedule equals repeated te_clock_add, an all-equal schedule
lands within 1 ulp of te_clock_add_ticks, the graph key compares values as bits) and the launch plan of a fused request with a
schedule (csrc/step_variant.hpp, plan_step: one launch where the traits allow it, tick by tick under each of the listed
conditions, a request type without the member plans as before)."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("program,ok", [("dt_schedule_test", "dt schedule tests ok"),
                                        ("dt_schedule_plan_host_test", "dt schedule plan host test ok")])
def test_host_program(tmp_path, program, ok):
    exe = str(tmp_path / program)
    src = os.path.join(ROOT, "tests", "host", program + ".cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ok in out.stdout
