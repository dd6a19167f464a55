"""Generate tests/golden/crater_fields.npz: crater lists and the reference's own float64 terrain.

Run on a CPU machine that has the read-only reference tree (never on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_crater_golden.py <reference root>

(or MPPI_REFERENCE_ROOT=<reference root>).  The reference's Surface.create_surface
(thesis_master/warp_implementation/MPPI_isaac.py:307-356) is imported from that tree and called; the
modules it imports that are not installed (warp, cv2, ...) are stubbed with MagicMock, none of them is
touched by create_surface.  Only data goes into the file: per case k the crater rows
craters_k [n, 4] = (cx, cy, height, width), grid_k, half_width_k and Z_k, the float64 array the
reference returned.  No reference program text is stored.

Cases (drawn in this order from one RandomState(5); per crater cx, cy ~ U(-hw, hw), height ~
U(0.6, 4.5), width ~ U(0.5, 3.0), in that order):

    grid  half-width  craters
      17        0.85        1   one ragged MFMA tile, 2 terms (the term count is padded)
     130        6.5         3   ragged workgroup tile, 6 terms
     257       12.85       33   several tiles plus a one-cell edge, 66 terms
     130        6.5      1100   2200 terms: crosses every LDS chunk boundary of the factor tables
"""
from __future__ import annotations

import importlib
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(17, 0.85, 1), (130, 6.5, 3), (257, 12.85, 33), (130, 6.5, 1100)]


def reference_surface(root):
    """The reference's Surface class, its missing imports stubbed."""
    sys.dont_write_bytecode = True
    wi = os.path.join(root, "thesis_master", "warp_implementation")
    for p in (root, wi):
        if p not in sys.path:
            sys.path.insert(0, p)
    for _ in range(64):   # stub whatever fails to import, one module per attempt
        try:
            return importlib.import_module("MPPI_isaac").Surface
        except ImportError as e:
            if not e.name or e.name in sys.modules:
                raise
            sys.modules[e.name] = MagicMock()
    raise RuntimeError("MPPI_isaac does not import")


def draw_cases():
    rng = np.random.RandomState(5)
    out = []
    for grid, hw, n in CASES:
        rows = np.empty((n, 4), np.float64)
        for k in range(n):
            rows[k, 0] = rng.uniform(-hw, hw)
            rows[k, 1] = rng.uniform(-hw, hw)
            rows[k, 2] = rng.uniform(0.6, 4.5)
            rows[k, 3] = rng.uniform(0.5, 3.0)
        out.append((grid, hw, rows))
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MPPI_REFERENCE_ROOT")
    if not root or not os.path.isdir(root):
        sys.exit("usage: make_crater_golden.py <reference root>")
    Surface = reference_surface(os.path.abspath(root))
    data = {"cases": np.int64(len(CASES))}
    for k, (grid, hw, rows) in enumerate(draw_cases()):
        s = Surface.__new__(Surface)
        s.half_width = hw
        s.grid_size = grid
        bumps = [((float(r[0]), float(r[1])), float(r[2]), float(r[3])) for r in rows]
        _, _, Z = s.create_surface(bumps)
        assert Z.dtype == np.float64 and Z.shape == (grid, grid)
        data[f"craters_{k}"] = rows
        data[f"grid_{k}"] = np.int64(grid)
        data[f"half_width_{k}"] = np.float64(hw)
        data[f"Z_{k}"] = Z
    path = os.path.join(HERE, "crater_fields.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
