"""CPU: the step engine's slot policies and owning handles (csrc/mppi_slots.h, csrc/mppi_handles.h).

Compiles tests/native/slot_policy_check.cpp for the host with AddressSanitizer and UBSan and runs it:
the normals-slot victim and search agree with a literal restatement of the rule over every state of
the three slots, the tail ring's next slot follows the deferred tail when there is one, and a handle
releases its resource exactly once (after a move, a move-assignment onto a live handle, a reset and
a grow) and never a borrowed one.  The headers need no HIP header here (a counting fake stands in
for the runtime), and nothing is loaded into Python.
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


def test_slot_policies_and_handles(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "slot_policy_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", os.path.join(HERE, "native", "slot_policy_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    t0 = time.monotonic()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    dt = time.monotonic() - t0
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "slot policy ok" in out.stdout
    assert dt < 1.0, f"the check took {dt:.2f} s"
