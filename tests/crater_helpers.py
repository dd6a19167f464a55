"""Shared by the crater-field DEM tests: the fixture of tests/golden/make_crater_golden.py (the reference's
own Surface.create_surface output) and the acceptance rule of a built DEM against it."""
from __future__ import annotations

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crater_fields.npz")
MAX_DIFFERING_SHARE = 1e-3


@functools.lru_cache(maxsize=None)
def crater_cases():
    """[(grid, half_width, craters [n, 4] float64, float32(reference Z))], loaded once; read-only arrays."""
    d = np.load(GOLDEN)
    out = []
    for k in range(int(d["cases"])):
        cr = np.ascontiguousarray(d[f"craters_{k}"], np.float64)
        ref = d[f"Z_{k}"].astype(np.float32)
        cr.setflags(write=False)
        ref.setflags(write=False)
        out.append((int(d[f"grid_{k}"]), float(d[f"half_width_{k}"]), cr, ref))
    return out


CASE_IDS = ["17-1", "130-3", "257-33", "130-1100"]


def assert_dem_close(got, ref32, what=""):
    """Every cell within one float32 ulp of ref32 (floor 2^-126: a conversion that flushes a float32
    denormal), and at most 1e-3 of the cells differing at all.  Returns the number that differ."""
    got = np.asarray(got)
    ref32 = np.asarray(ref32)
    assert got.dtype == np.float32 and ref32.dtype == np.float32 and got.shape == ref32.shape, (got.dtype, got.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite heights"
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bound = np.maximum(np.spacing(np.abs(ref32)).astype(np.float64), 2.0 ** -126)
    worst = int(np.argmax(err - bound))
    differing = int(np.count_nonzero(got != ref32))
    print(f"{what}: {differing} of {got.size} cells differ, max |err| {err.max():.3e}")
    assert (err <= bound).all(), (f"{what}: cell {np.unravel_index(worst, got.shape)} got {got.flat[worst]!r} "
                                  f"ref {ref32.flat[worst]!r} (more than one float32 ulp)")
    assert differing <= MAX_DIFFERING_SHARE * got.size, f"{what}: {differing} of {got.size} cells differ"
    return differing
