"""CPU: the hazard costmap's rule and host side.

scene.hazard_occupancy, the package's numpy statement of the rule, against the independent restatement
of tests/hazard_refs.py (oracle normal, tables written out again, brute-force distance), bit for bit;
the cell counts of the crater fixtures; and csrc/mppi_hazard.h (tables, T, refusals, tiling) driven by
tests/native/hazard_tables_check.cpp, a stand-alone program built with AddressSanitizer and UBSan.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hazard_refs as HR
from mppi_amd import scene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc")


def _geom(Z, hw):
    return -hw, -hw, 2.0 * hw / Z.shape[1]


@pytest.fixture(scope="module")
def crater192():
    return scene.crater_dem(192, 75.0)


@pytest.mark.parametrize("deg,n0,n1", [(10.0, 140, 231), (15.0, 81, 160), (20.0, 23, 62), (30.0, 0, 0)])
def test_crater_fixture_counts(crater192, deg, n0, n1):
    x_min, y_min, res = _geom(crater192, 75.0)
    H0, H1 = scene.hazard_occupancy(crater192, x_min, y_min, res, 24, 75.0, deg, 1, 7.0)
    assert HR.threshold(7.0, 24, 75.0) == 1
    assert (int(H0.sum()), int(H1.sum())) == (n0, n1)
    W0, W1 = HR.occupancy(crater192, x_min, y_min, res, 24, 75.0, deg, 1, 7.0)
    assert np.array_equal(H0, W0) and np.array_equal(H1, W1)


CASES = HR.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_statement_equals_restatement(name):
    Z, x_min, y_min, res, size, hw, deg, mc, infl = CASES[name]
    H0, H1 = scene.hazard_occupancy(Z, x_min, y_min, res, size, hw, deg, mc, infl)
    W0, W1 = HR.occupancy(Z, x_min, y_min, res, size, hw, deg, mc, infl)
    assert H0.dtype == bool and H0.shape == (size, size)
    assert np.array_equal(H0, W0), name
    assert np.array_equal(H1, W1), name
    assert not (H0 & ~H1).any()
    if name == "min65":
        assert not H0.any() and not H1.any()     # 64 DEM cells per costmap cell: none can collect 65
    if name == "flat":
        assert not H0.any()
    if name == "nonfinite":
        st = scene.hazard_steep(Z, res, deg)
        assert st[Z.shape[0] // 3, Z.shape[1] // 2] and st[0, 0] and st[-1, -1] and st[-2, -2]
    if name == "t2_160_33":
        assert HR.threshold(infl, size, hw) == 2


def test_tables_equal_restatement():
    for rows, cols, x_min, y_min, res, size, hw in ((96, 130, -31.0, -17.5, 0.5, 33, 30.0),
                                                    (160, 160, -75.0, -75.0, 150.0 / 160, 33, 75.0),
                                                    (5, 7, 100.0, 3.0, 0.1, 24, 10.0)):
        ci, rj = scene.hazard_tables(rows, cols, x_min, y_min, res, size, hw)
        wi, wj = HR.tables(rows, cols, x_min, y_min, res, size, hw)
        assert np.array_equal(ci, wi) and np.array_equal(rj, wj)


def test_hazard_value():
    from mppi_amd import _lib
    h = _lib.make_hazard(scene.Hazard(15.0), 1.2)
    assert (h.max_slope_deg, h.min_cells, h.reserved) == (15.0, 1, 0) and h.inflate == np.float32(1.2 + 0.1)
    h = _lib.make_hazard({"max_slope_deg": 20, "inflate": 0.0, "min_cells": 3}, 1.2)
    assert (h.max_slope_deg, h.inflate, h.min_cells) == (20.0, 0.0, 3)
    assert _lib.make_hazard(None, 1.2) is None
    with pytest.raises(ValueError):
        _lib.make_hazard({"slope": 3}, 1.2)


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or "", shutil.which("g++") or ""):
        if c and os.path.exists(c):
            return c
    return None


def test_hazard_header_native(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no C++ compiler (the library's own build needs /opt/rocm/llvm/bin/clang++)"
    exe = str(tmp_path / "hazard_tables_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}",
           os.path.join(HERE, "native", "hazard_tables_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "hazard tables ok" in out.stdout


def test_the_header_includes_no_hip():
    text = open(os.path.join(CSRC, "mppi_hazard.h")).read()
    assert "#include <hip" not in text and '#include "mppi_kernels.h"' not in text and '#include "mppi_ctx.h"' not in text
