"""CPU: the bookkeeping of a batch's per-episode scenes and trajectory counts (csrc/mppi_batch_scene.h).

Compiles tests/native/batch_scene_check.cpp for the host with AddressSanitizer and UBSan and runs it
as a stand-alone program: slots are set, replaced and freed, a held slot is not freed, a geometry
mismatch names the slot, blocks_e = ceil(K_e / 256) for K_e = 1, 256, 257, 512, and the kernels get
no table while no episode in use holds anything (again after the last holder resets).  The header
needs no HIP header, and nothing is loaded into Python.
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


def test_batch_scene_book(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "batch_scene_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", os.path.join(HERE, "native", "batch_scene_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    t0 = time.monotonic()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    dt = time.monotonic() - t0
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "batch scene book ok" in out.stdout
    assert dt < 1.0, f"the check took {dt:.2f} s"


def test_the_header_includes_no_hip():
    text = open(os.path.join(CSRC, "mppi_batch_scene.h")).read()
    assert "#include <hip" not in text and '#include "mppi_kernels.h"' not in text
