"""CPU: the bookkeeping of a batch's task list (csrc/mppi_batch_tasks.h).

Compiles tests/native/batch_tasks_check.cpp for the host with AddressSanitizer and UBSan and runs it
as a stand-alone program: every refusal of a listed task names its field, the log base rows are the
prefix sums of the caps (disjoint, gapless, exact past 2^31), blocks = ceil(K / 256), the kernels get
the variant and the scene table only when a listed task needs them, the projections come from the
list, a slot or variant row a listed task holds is reported held, and campaign_makespan equals a
lane-by-lane simulation on random lists.  The header needs no HIP header, and nothing is loaded into
Python.
"""
import os
import shutil
import subprocess
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc")


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or "", shutil.which("g++") or ""):
        if c and os.path.exists(c):
            return c
    return None


def test_batch_task_book(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "batch_tasks_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", os.path.join(HERE, "native", "batch_tasks_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    t0 = time.monotonic()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    dt = time.monotonic() - t0
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "batch task book ok" in out.stdout
    assert dt < 2.0, f"the check took {dt:.2f} s"


def test_the_header_includes_no_hip():
    text = open(os.path.join(CSRC, "mppi_batch_tasks.h")).read()
    assert "#include <hip" not in text and '#include "mppi_kernels.h"' not in text
    # and the one project header it includes has none either
    assert '#include "mppi_batch_scene.h"' in text
    scene = open(os.path.join(CSRC, "mppi_batch_scene.h")).read()
    assert "#include <hip" not in scene and '#include "mppi_kernels.h"' not in scene
