"""TEST INFRASTRUCTURE: the hazard-costmap rule restated from the oracles alone.

Independent of mppi_amd.scene.hazard_occupancy: the normal is oracle.mppi_ref.normal_on_grid on the
clamped corners, the two tables are written out again from the rule, the inflation is a threshold on
oracle.costmap_ref.edt_bruteforce, and the map is composed from the costmap oracle's own pieces
(chamfer_l2_5x5 / cv_normalize_minmax / cv_power for the chamfer metrics, edt / scale for the exact
one), the way tests/test_gpu_costmap.py holds the rock-only build.
"""
import math

import numpy as np

from oracle import costmap_ref as CR
from oracle import mppi_ref as R

F32 = np.float32


def steep_cells(Z, res, max_slope_deg):
    Z = np.asarray(Z, F32)
    rows, cols = Z.shape
    j, i = np.mgrid[0:rows, 0:cols]
    j1 = np.minimum(j + 1, rows - 1)
    i1 = np.minimum(i + 1, cols - 1)
    q = (Z[j, i], Z[j, i1], Z[j1, i], Z[j1, i1])
    with np.errstate(all="ignore"):
        nz = R.normal_on_grid(q, F32(res))[2]
    assert nz.dtype == F32
    c = F32(math.cos(float(F32(max_slope_deg)) * math.pi / 180.0))
    with np.errstate(invalid="ignore"):
        return np.logical_not(nz >= c)


def tables(rows, cols, x_min, y_min, res, size, hw):
    rc = 2 * float(hw) / size
    x_min, y_min, res = float(F32(x_min)), float(F32(y_min)), float(F32(res))
    ci, rj = [], []
    for i in range(cols):
        v = math.floor((x_min + (i + 0.5) * res + float(hw)) / rc)
        ci.append(v if 0 <= v < size else -1)
    for j in range(rows):
        v = math.floor((float(hw) - (-y_min - (j + 0.5) * res)) / rc)
        rj.append(v if 0 <= v < size else -1)
    return np.array(ci, np.int64), np.array(rj, np.int64)


def threshold(inflate, size, hw):
    return int(math.floor((float(F32(inflate)) / (2 * float(hw) / size)) ** 2))


def occupancy(Z, x_min, y_min, res, size, hw, max_slope_deg, min_cells=1, inflate=0.0):
    """(H0, H1) of the rule."""
    st = steep_cells(Z, res, max_slope_deg)
    ci, rj = tables(st.shape[0], st.shape[1], x_min, y_min, res, size, hw)
    cnt = np.zeros((size, size), np.int64)
    for j, i in zip(*np.nonzero(st)):
        if rj[j] >= 0 and ci[i] >= 0:
            cnt[rj[j], ci[i]] += 1
    H0 = cnt >= min_cells
    d = CR.edt_bruteforce(H0)
    if d is None:
        return H0, np.zeros_like(H0)
    T = threshold(inflate, size, hw)
    d2 = np.rint(d * d).astype(np.int64)      # edt_bruteforce returns sqrt of the integer
    return H0, d2 <= T


def expected_mask(H0, H1, discs):
    return (H0.astype(np.uint8) | (H1.astype(np.uint8) << 1) | (discs.astype(np.uint8) << 2)).astype(np.uint8)


def expected_map(occ, power, metric):
    """The costmap of an occupancy, for the metric names of mppi_amd._lib.COSTMAP_METRICS."""
    if metric in ("chamfer", "chamfer_raster"):
        return CR.cv_power(CR.cv_normalize_minmax(CR.chamfer_l2_5x5(occ)), power)
    assert metric == "exact"
    out = CR.scale(CR.edt(occ), power)
    return np.ones(occ.shape, F32) if out is None else out


def expected_build(Z, x_min, y_min, res, obstacles, origin, size, hw, r_robot, power, metric, max_slope_deg,
                   min_cells=1, inflate=0.0):
    """(map, mask) of a hazard build."""
    H0, H1 = occupancy(Z, x_min, y_min, res, size, hw, max_slope_deg, min_cells, inflate)
    discs = CR.raster(obstacles, origin, size, hw, r_robot)
    return expected_map(H1 | discs, power, metric), expected_mask(H0, H1, discs)


def patchy(rows, cols, seed):
    rng = np.random.RandomState(seed)
    Z = (0.4 * rng.standard_normal((rows, cols))).astype(np.float32)
    Z[rows // 3: rows // 3 + 2, cols // 2: cols // 2 + 3] = np.nan
    Z[0, 0] = np.inf
    Z[-1, -1] = -np.inf
    Z[-1, cols // 4] = 9.0       # the last row and column: the clamped corners
    Z[rows // 2, -1] = -9.0
    return Z


def near_limit(rows, cols, res, deg):
    """A ramp along x whose slope is the limit's to within a few float32 ulps, a little more or less from
    row pair to row pair: the cells where only the full normal decides."""
    s = math.tan(math.radians(deg)) * (1.0 + 2e-7 * (np.arange(rows) // 2 - rows // 4))
    return (s[:, None] * (np.arange(cols) * res)[None, :]).astype(F32)


def cases():
    """The geometry and edge cases both the host and the GPU tests run (inputs only)."""
    from mppi_amd import scene
    return {
        # name: (Z, x_min, y_min, res, size, hw, deg, min_cells, inflate)
        "t2_160_33": (scene.crater_dem(160, 75.0), -75.0, -75.0, 150.0 / 160, 33, 75.0, 12.0, 1, 7.0),
        "min3": (scene.crater_dem(192, 75.0), -75.0, -75.0, 150.0 / 192, 24, 75.0, 10.0, 3, 0.0),
        "min64": (scene.crater_dem(192, 75.0), -75.0, -75.0, 150.0 / 192, 24, 75.0, 5.0, 64, 7.0),
        "min65": (scene.crater_dem(192, 75.0), -75.0, -75.0, 150.0 / 192, 24, 75.0, 5.0, 65, 7.0),
        "offcentre_96x130": (patchy(96, 130, 1), -31.0, -17.5, 0.5, 33, 30.0, 35.0, 2, 4.0),
        "small_hw": (scene.crater_dem(192, 75.0), -75.0, -75.0, 150.0 / 192, 24, 30.0, 12.0, 1, 3.0),
        "cols191": (scene.crater_dem(192, 75.0)[:, :191], -75.0, -75.0, 150.0 / 192, 24, 75.0, 12.0, 1, 7.0),
        "cols193": (np.pad(scene.crater_dem(192, 75.0), ((0, 0), (0, 1)), mode="edge"), -75.0, -75.0, 150.0 / 192, 24,
                    75.0, 12.0, 1, 7.0),
        "dem2x2": (np.array([[0.0, 50.0], [0.0, 0.0]], np.float32), -75.0, -75.0, 75.0, 24, 75.0, 20.0, 1, 13.0),
        "flat": (np.full((64, 48), 2.5, np.float32), -20.0, -30.0, 1.0, 24, 40.0, 1.0, 1, 5.0),
        "nonfinite": (patchy(64, 64, 2), -16.0, -16.0, 0.5, 24, 16.0, 60.0, 1, 0.0),
        # two column tiles of the count kernel, the halo column crossing waves and tiles
        "wide_8x1100": (patchy(8, 1100, 3), -55.0, -0.4, 0.1, 33, 60.0, 80.0, 2, 0.0),
        "near_limit": (near_limit(48, 64, 0.5, 20.0), -16.0, -12.0, 0.5, 24, 16.0, 20.0, 1, 0.0),
        "finer_costmap": (scene.crater_dem(40, 75.0), -75.0, -75.0, 3.75, 128, 75.0, 12.0, 1, 2.0),
    }
