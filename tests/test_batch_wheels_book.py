"""CPU: which device tables of the wheel log, the wheel slope chain and the path metrics exist when
(csrc/mppi_batch_wheels.h, the book mppi_capi_batch.cpp allocates, frees and launches by).

Compiles tests/native/batch_wheels_check.cpp for the host with AddressSanitizer and UBSan and runs it as
a stand-alone program: every combination of keep_log, wheel_log, scored, slope mode and metrics for runs,
task lists and tracking, who owns the log's parallel array, and the refusals.  Nothing is loaded into
Python.
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


def test_batch_wheels_book(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "batch_wheels_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", os.path.join(HERE, "native", "batch_wheels_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "batch wheels book ok" in out.stdout


def test_the_c_api_decides_through_the_book():
    """mppi_capi_batch.cpp keeps no option flag of its own: every decision reads the book."""
    src = open(os.path.join(CSRC, "mppi_capi_batch.cpp")).read()
    assert '#include "mppi_batch_wheels.h"' in src and "BatchWheelBook wbook;" in src
    for gone in ("opt_slope", "opt_metrics", "list_wheel_log", "list_slope_wheels", "list_metrics", "trk_metrics",
                 "trk_slope_wheels", "b->wheel_log", "b->log_wheels"):
        assert gone not in src, gone
    for used in (".take_run()", ".take_list(scored, keep_log)", ".take_tracking(", "wbook.clear_list()",
                 "wbook.clear_tracking()", "wbook.can_score_wheels(", "wbook.set_wheel_log(", "wbook.set_score_options("):
        assert used in src, used
