"""tests/c_abi/select_soonest_test.c: a plain C caller (gcc -std=c99, no HIP headers) of the three host-visible forms of the
k-soonest selection, behind ticks with the query on a two-model manager.  The program prints the query's outputs and the rows it
got (doubles as hexadecimal floats); here they are held against NumPy: slots, ids, delta bits and pose rows equal."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_cpp_example_of_the_interceptors_loop(tmp_path):
    """examples/soonest_crossings.cpp: tick + query, the gate, the selection on the device, the k rows printed in order"""
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "soonest_crossings")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "examples", "soonest_crossings.cpp"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, os.path.join(ROOT, "models"), "3000", "12", "8"], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "soonest crossings example ok" in out.stdout and "ONE launch" in out.stdout
    m = re.search(r"after the last tick (\d+) of k = 8 rows", out.stdout)
    assert m and 0 < int(m.group(1)) <= 8, out.stdout        # the loop did select converged crossings
    assert len(re.findall(r"crosses in", out.stdout)) == int(m.group(1))


def test_plain_c_caller_of_the_selection(tmp_path):
    libdir = os.path.join(ROOT, "target_estimation_amd", "lib")
    exe = str(tmp_path / "select_soonest_test")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include", "target_estimation_amd"),
                           os.path.join(ROOT, "tests", "c_abi", "select_soonest_test.c"), "-o", exe,
                           "-L", libdir, "-ltarget_estimation_amd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, model_path("uniform_acceleration")], capture_output=True, text=True, timeout=60)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr
    assert "select soonest test ok" in out.stdout
    sizes, entries, rows, counts = {}, {}, {}, {}
    for ln in out.stdout.splitlines():
        w = ln.split()
        if not w:
            continue
        if w[0] == "N":
            sizes[int(w[1])] = int(w[2])
        elif w[0] == "E":
            entries[(int(w[1]), int(w[2]))] = (int(w[3]), float.fromhex(w[4]), [float.fromhex(x) for x in w[5:12]])
        elif w[0] == "COUNT":
            counts[w[1]] = int(w[2])
        elif w[0] == "ROW":
            rows.setdefault(w[1], []).append((int(w[3]), int(w[4]), int(w[5]), float.fromhex(w[6]), [float.fromhex(x) for x in w[7:14]]))
    assert sizes == {0: 300, 1: 70}
    d = [np.array([entries[(b, i)][1] for i in range(sizes[b])]) for b in (0, 1)]
    ids = [np.array([entries[(b, i)][0] for i in range(sizes[b])], dtype=np.uint64) for b in (0, 1)]
    pose = [np.array([entries[(b, i)][2] for i in range(sizes[b])]) for b in (0, 1)]
    assert (d[1] == -1).all() and (d[0] >= 0).sum() > 16          # uniform_velocity never crosses; the accelerating targets do
    filler = [0, 0, 0, 0, 0, 0, 1.0]

    def check(form, sel_batch, sel_slot, k, with_pose):
        got = rows[form]
        assert len(got) == k and counts[form] == len(sel_slot) == min(k, len(sel_slot))
        for i, (gid, gb, gs, gd, gp) in enumerate(got):
            if i < len(sel_slot):
                b, s = int(sel_batch[i]), int(sel_slot[i])
                assert (gid, gb, gs) == (int(ids[b][s]), b, s), (form, i)
                assert _bits(gd) == _bits(d[b][s]), (form, i)
                if with_pose:
                    assert np.array_equal(_bits(gp), _bits(pose[b][s])), (form, i)
            else:
                assert (gid, gb, gs, gd, gp) == (0xFFFFFFFF, -1, -1, -1.0, filler), (form, i)

    # the batch calls: batch 0, mask i % 3 != 0, k = 5, ordered by (delta, slot)
    ok = np.arange(300) % 3 != 0
    cand = np.flatnonzero(ok & (d[0] >= 0.0) & (d[0] <= np.inf))
    sel = cand[np.lexsort((cand, d[0][cand]))][:5]
    check("batch_dev", np.zeros(len(sel), int), sel, 5, True)
    check("batch", np.zeros(len(sel), int), sel, 5, True)
    # the manager call: both batches, no mask, k = 16, ordered by (delta, batch, slot)
    alld = np.concatenate(d)
    allb = np.concatenate([np.full(300, 0), np.full(70, 1)])
    alls = np.concatenate([np.arange(300), np.arange(70)])
    cand = np.flatnonzero((alld >= 0.0) & (alld <= np.inf))
    sel = cand[np.lexsort((cand, allb[cand], alld[cand]))][:16]
    check("manager", allb[sel], alls[sel], 16, False)
