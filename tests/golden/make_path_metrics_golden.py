"""Generate tests/golden/path_metrics.npz: executed paths and the reference's own compute_path_metrics.

Run on a CPU machine that has the read-only reference tree (never on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_path_metrics_golden.py <reference root>

(or MPPI_REFERENCE_ROOT=<reference root>).  The reference's compute_path_metrics
(thesis_master/warp_implementation/MPPI_isaac.py:231-256) is imported from that tree and called; the
modules it imports that are not installed (warp, cv2, ...) are stubbed with MagicMock, none of them is
touched by the function.  Only data goes into the file: per case k the waypoints path_k [L, 3] float32
(what a log row holds) and metrics_k [4] float64 = (length, angle_up, angle_down, distance_up), the four
numbers the reference returned for path_k widened to float64.  No reference program text is stored.

Cases, drawn in this order from one RandomState(11):

    random walks of 0, 1, 21, 22, 23, 41, 42, 43, 61, 62 and 3500 rows: steps of ~0.09 m in x, y with a
        slowly varying slope, so every longer path climbs and descends within one run;
    `zero_segment`, 43 rows: rows 0 .. 21 are one repeated pose (the first segment has length 0: no angle,
        no climb), then a climb;
    `level_segment`, 43 rows: rows 0 and 21 have the same z (s.z == 0: the angle is 0 and goes to
        angle_down as |0|, nothing to distance_up), the second segment descends;
    `vertical`, 22 rows: x, y constant, z rising: the arctangent's argument is (s.z, 0).
"""
from __future__ import annotations

import importlib
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (0, 1, 21, 22, 23, 41, 42, 43, 61, 62, 3500)


def reference_metrics(root):
    """The reference's compute_path_metrics, its module's missing imports stubbed."""
    sys.dont_write_bytecode = True
    wi = os.path.join(root, "thesis_master", "warp_implementation")
    for p in (root, wi):
        if p not in sys.path:
            sys.path.insert(0, p)
    for _ in range(64):   # stub whatever fails to import, one module per attempt
        try:
            return importlib.import_module("MPPI_isaac").compute_path_metrics
        except ImportError as e:
            if not e.name or e.name in sys.modules:
                raise
            sys.modules[e.name] = MagicMock()
    raise RuntimeError("MPPI_isaac does not import")


def draw_cases():
    rng = np.random.RandomState(11)
    out = []
    for L in LENGTHS:
        step = rng.normal(0.0, 0.09, size=(L, 2))
        slope = np.sin(np.arange(L) / 17.0 + rng.uniform(0, 6.0)) * 0.03 + rng.normal(0.0, 0.004, size=L)
        p = np.zeros((L, 3))
        if L:
            p[:, :2] = np.cumsum(step, 0) + rng.uniform(-60, 60, size=2)
            p[:, 2] = np.cumsum(slope) + rng.uniform(0, 3.0)
        out.append((f"walk{L}", p.astype(np.float32)))
    z = np.zeros((43, 3))
    z[:22] = (3.25, -7.5, 1.125)
    z[22:, 0] = 3.25 + 0.1 * np.arange(1, 22)
    z[22:, 1] = -7.5
    z[22:, 2] = 1.125 + 0.02 * np.arange(1, 22)
    out.append(("zero_segment", z.astype(np.float32)))
    lv = np.zeros((43, 3))
    lv[:, 0] = -12.0 + 0.1 * np.arange(43)
    lv[:, 1] = 4.0 + 0.05 * np.arange(43)
    lv[:, 2] = 2.0 + 0.01 * np.sin(np.arange(43))
    lv[21, 2] = lv[0, 2]
    lv[41, 2] = lv[20, 2] - 0.75
    out.append(("level_segment", lv.astype(np.float32)))
    vt = np.zeros((22, 3))
    vt[:, 0], vt[:, 1] = 1.5, -2.5
    vt[:, 2] = 0.03 * np.arange(22)
    out.append(("vertical", vt.astype(np.float32)))
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MPPI_REFERENCE_ROOT")
    if not root or not os.path.isdir(root):
        sys.exit("usage: make_path_metrics_golden.py <reference root>")
    metrics = reference_metrics(os.path.abspath(root))
    cases = draw_cases()
    data = {"cases": np.int64(len(cases)), "names": np.array([n for n, _ in cases])}
    for k, (name, p) in enumerate(cases):
        # the waypoints a log row holds are float32; the reference computes in float64 on what it is given
        got = metrics(p.astype(np.float64))
        data[f"path_{k}"] = p
        data[f"metrics_{k}"] = np.array([float(g) for g in got], np.float64)
    path = os.path.join(HERE, "path_metrics.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
