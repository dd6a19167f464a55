"""CPU: the "no log" mode of a batch's task book (csrc/mppi_batch_tasks.h), the book of a scored list
that keeps no log (mppi_batch_set_tasks_scored with keep_log = 0).

Compiles tests/native/batch_online_check.cpp for the host with AddressSanitizer and UBSan and runs it
as a stand-alone program: the book accepts caps whose sum the logged book refuses, hands out no base
rows, and keeps every other rule (refusals, held slots and variant rows, scene records, projections).
Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc")


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or "", shutil.which("g++") or ""):
        if c and os.path.exists(c):
            return c
    return None


def test_batch_online_book(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "batch_online_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", os.path.join(HERE, "native", "batch_online_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "batch online book ok" in out.stdout
