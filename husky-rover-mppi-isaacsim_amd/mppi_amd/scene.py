"""Synthetic scene recipes (the reference's .npy scene blobs are not in the repo).

SURVEY.md §0.5 / §8(d): ``costmap_750_*.npy`` and ``test_nathan.npy`` are
missing (.MISSING_LARGE_BLOBS), so every scene is regenerated from the
reference's own recipes:

* DEM craters: ``Surface.create_surface`` (thesis_master/warp_implementation/
  MPPI_isaac.py:307-356) with the 9-crater list of MPPI_OO_current.py:730-740,
  on the 1500^2 @ 0.1 m grid of MPPI_OO_current.py:209-213.
* Costmap: 750 random discs (MPPI_OO_current.py:721-725, RandomState(99)),
  inflated by robot radius + 0.2 (MPPI_OO_current.py:293), Euclidean distance
  transform, min-max normalise, ``(1 - d)**10`` (create_costmap.py:15-28).
  cv2.distanceTransform(DIST_L2, 5) is not available; scipy's exact EDT is used
  instead (parity of the costmap *builder* is unpinned; the costmap is an input
  of the hot path).

Host-side scene construction only: this is not on the MPPI step path.
"""
from __future__ import annotations

import numpy as np

# MPPI_OO_current.py:730-740 (commented scene block)
BUMPS_9 = [
    ((-2.7, -19.0), 3.4, 12.23),
    ((-0.57, -0.05), 4.39, 11.52),
    ((-48.56, 12.78), 3.6, 12.4),
    ((-27.89, 38.56), 4.0, 12.7),
    ((-50.12, 19.34), 3.7, 13.0),
    ((20.45, -48.78), 4.4, 12.9),
    ((-20.67, -40.12), 4.2, 12.9),
    ((42.78, 21.56), 4.5, 12.7),
    ((-36.12, -33.34), 3.9, 13.0),
]


def crater_dem(grid_size, half_width, bumps=BUMPS_9, scale=1.0):
    """Surface.create_surface (MPPI_isaac.py:307-356): crater = rim gaussian minus bowl gaussian."""
    x = np.linspace(-half_width, half_width, grid_size)
    X, Y = np.meshgrid(x, x)
    Z = np.zeros_like(X)
    for (cx, cy), h, w in bumps:
        cx, cy, w = cx * scale, cy * scale, w * scale
        r2 = (X - cx) ** 2 + (Y - cy) ** 2
        Z += (h - 0.5) * np.exp(-r2 / (2 * w ** 2))
        Z -= (h + 0.5) * np.exp(-r2 / (2 * (w / 2) ** 2))
    return Z.astype(np.float32)


def crater_rows(bumps):
    """Crater list -> contiguous float64 [n, 4] rows (cx, cy, height, width); n may be 0.  Accepted: the
    reference's own shape [((cx, cy), height, width), ...] (MPPI_isaac.py:318), an (n, 4) array, or a
    CraterField."""
    if isinstance(bumps, CraterField):
        return bumps.rows
    if isinstance(bumps, np.ndarray):
        a = np.asarray(bumps, np.float64)
        if a.size and (a.ndim != 2 or a.shape[1] != 4):
            raise ValueError(f"craters: an array must be (n, 4) rows (cx, cy, height, width), got {a.shape}")
        return np.ascontiguousarray(a.reshape(-1, 4))
    rows = []
    for k, b in enumerate(bumps):
        if len(b) == 3 and np.ndim(b[0]) == 1:
            (cx, cy), h, w = b
        elif len(b) == 4:
            cx, cy, h, w = b
        else:
            raise ValueError(f"crater {k}: expected ((cx, cy), height, width) or (cx, cy, height, width), got {b!r}")
        rows.append((float(cx), float(cy), float(h), float(w)))
    return np.ascontiguousarray(np.asarray(rows, np.float64).reshape(-1, 4))


class CraterField:
    """A crater field as a value: the rows (cx, cy, height, width) and an optional base terrain
    (float32 heights the craters are added to).  Wherever the controller takes a DEM array it takes
    one of these and builds the heights on the device (Engine.build_dem / Batch.build_dem)."""

    def __init__(self, bumps, base=None):
        self.rows = crater_rows(bumps)
        self.base = None if base is None else np.ascontiguousarray(base, dtype=np.float32)

    def __len__(self):
        return self.rows.shape[0]

    def __repr__(self):
        return f"CraterField({len(self)} craters{'' if self.base is None else ', base ' + str(self.base.shape)})"

    def dem(self, grid_size, half_width):
        """The heights on the host (crater_dem_separable)."""
        return crater_dem_separable(grid_size, half_width, self.rows, self.base)


def crater_dem_separable(grid_size, half_width, bumps, base=None):
    """Surface.create_surface (MPPI_isaac.py:307-320) as the separable float64 sum the device builder
    computes: x = linspace(-hw, hw, grid), row i at y_i = x_i; per crater the terms
    (a, s) = (height - 0.5, 2 width^2) and (-(height + 0.5), 2 (width/2)^2); R[i, t] = a_t exp(-((y_i -
    cy_t)^2) / s_t), C[t, j] = exp(-((x_j - cx_t)^2) / s_t); Z = R @ C in float64, plus the float32 base
    widened to float64, rounded once to float32.  No crater is culled.  The CPU yardstick of
    mppi_build_dem; not bitwise crater_dem (exp of a sum against a product of exps, the order of the sum)."""
    grid_size = int(grid_size)
    rows = crater_rows(bumps)
    x = np.linspace(-half_width, half_width, grid_size)
    Z = np.zeros((grid_size, grid_size), np.float64)
    if rows.shape[0]:
        cx, cy, h, w = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
        a = np.stack([h - 0.5, -(h + 0.5)], 1).reshape(-1)                 # [2n] rim, bowl per crater
        s = np.stack([2 * w ** 2, 2 * (w / 2) ** 2], 1).reshape(-1)
        cx2, cy2 = np.repeat(cx, 2), np.repeat(cy, 2)
        R = a[None, :] * np.exp(-((x[:, None] - cy2[None, :]) ** 2) / s[None, :])   # [grid, 2n]
        Cf = np.exp(-((x[None, :] - cx2[:, None]) ** 2) / s[:, None])               # [2n, grid]
        Z = R @ Cf
    if base is not None:
        base = np.asarray(base, np.float32)
        if base.shape != Z.shape:
            raise ValueError(f"base: shape {base.shape}, the DEM's is {Z.shape}")
        Z = Z + base.astype(np.float64)
    return Z.astype(np.float32)


class Hazard:
    """Steep terrain as no-go cells of the obstacle costmap: DEM cells whose
    normal is steeper than max_slope_deg, counted into costmap cells (>= min_cells to qualify) and
    grown by `inflate` metres (None: r_robot + 0.1, the margin the reference gives its rocks).
    Wherever a costmap is built on the device (Engine / Batch / CostmapBuilder / rebuild_costmap,
    costmaps= entries) `hazard=` takes one of these or the same fields as a dict."""

    def __init__(self, max_slope_deg, inflate=None, min_cells=1):
        self.max_slope_deg = float(max_slope_deg)
        self.inflate = None if inflate is None else float(inflate)
        self.min_cells = int(min_cells)

    def __repr__(self):
        return f"Hazard(max_slope_deg={self.max_slope_deg}, inflate={self.inflate}, min_cells={self.min_cells})"


def hazard_steep(Z, resolution, max_slope_deg):
    """Steep DEM cells: cell (j, i) is steep iff !(nz >= c), nz the z component of the rollout's
    normal in that cell (projection_warp.py:129-151 on the corners (j, i), (j, i+1), (j+1, i),
    (j+1, i+1) clamped into the map, float32 in the reference's order) and
    c = float32(cos(max_slope_deg pi / 180)).  A NaN nz (non-finite heights) is steep."""
    Z = np.asarray(Z, np.float32)
    rows, cols = Z.shape
    r1 = np.minimum(np.arange(rows) + 1, rows - 1)
    c1 = np.minimum(np.arange(cols) + 1, cols - 1)
    q0, q1, q2, q3 = Z, Z[:, c1], Z[r1, :], Z[r1][:, c1]
    res = np.float32(resolution)
    hr = (-res) / np.float32(2.0)
    rs = res * res
    with np.errstate(all="ignore"):
        vx = hr * (((q1 - q0) - q2) + q3)
        vy = hr * (((q2 - q0) - q1) + q3)
        nz = rs / np.sqrt((vx * vx + vy * vy) + rs * rs)
        c = np.float32(np.cos(np.float64(np.float32(max_slope_deg)) * np.pi / 180.0))
        return ~(nz >= c)


def hazard_tables(rows, cols, x_min, y_min, resolution, size, half_width):
    """(ci[cols], rj[rows]): the costmap column / row the centre of a DEM column / row falls into,
    in the frame of the rollout's costmap lookup (column from x + half_width, row from
    -y + half_width), float64; -1 outside [0, size)."""
    hw = float(half_width)
    rc = 2 * hw / size
    x_min, y_min, res = (float(np.float32(v)) for v in (x_min, y_min, resolution))
    ci = np.floor((x_min + (np.arange(cols) + 0.5) * res + hw) / rc)
    rj = np.floor((hw - (-y_min - (np.arange(rows) + 0.5) * res)) / rc)
    ci = np.where((ci >= 0) & (ci < size), ci, -1).astype(np.int32)
    rj = np.where((rj >= 0) & (rj < size), rj, -1).astype(np.int32)
    return ci, rj


def hazard_occupancy(Z, x_min, y_min, resolution, size, half_width, max_slope_deg, min_cells=1, inflate=0.0):
    """The hazard rule on the CPU, the yardstick of mppi_build_costmap_hazard:
    returns (H0, H1), size x size bool.  H0: costmap cells that collected >= min_cells steep DEM
    cells (hazard_steep, hazard_tables).  H1: cells whose exact squared cell distance to the nearest
    H0 cell is <= T = floor((inflate / rc)^2), rc = 2 half_width / size (a disc dilation; H0 empty:
    H1 empty, inflate 0: H1 = H0)."""
    Z = np.asarray(Z, np.float32)
    size = int(size)
    steep = hazard_steep(Z, resolution, max_slope_deg)
    ci, rj = hazard_tables(Z.shape[0], Z.shape[1], x_min, y_min, resolution, size, half_width)
    ok = steep & (rj >= 0)[:, None] & (ci >= 0)[None, :]
    jj, ii = np.nonzero(ok)
    cnt = np.zeros((size, size), np.int64)
    np.add.at(cnt, (rj[jj], ci[ii]), 1)
    H0 = cnt >= int(min_cells)
    rc = 2 * float(half_width) / size
    T = int(np.floor((float(np.float32(inflate)) / rc) ** 2))
    if T == 0 or not H0.any():
        return H0, H0.copy()
    # vertical distance to the nearest H0 cell of the column, then the columns within sqrt(T)
    idx = np.arange(size, dtype=np.int64)[:, None]
    far = 4 * size
    up = np.maximum.accumulate(np.where(H0, idx, -far), axis=0)
    dn = np.minimum.accumulate(np.where(H0, idx, far)[::-1], axis=0)[::-1]
    g = np.minimum(idx - up, dn - idx)
    g2 = g * g
    H1 = np.zeros_like(H0)
    s = int(np.floor(np.sqrt(T)))
    while (s + 1) * (s + 1) <= T:
        s += 1
    for o in range(-min(s, size - 1), min(s, size - 1) + 1):
        lim = T - o * o
        if lim < 0:
            continue
        src = g2[:, max(0, -o):size - max(0, o)] <= lim      # H0 column x' = x - o reaches column x
        H1[:, max(0, o):size - max(0, -o)] |= src
    return H0, H1


def random_obstacles(n=750, seed=99, extent=50.0, r_max=0.4):
    """MPPI_OO_current.py:721-725: [x, y, r] with RandomState(seed)."""
    rng = np.random.RandomState(seed)
    return [[rng.uniform(-extent, extent), rng.uniform(-extent, extent), rng.uniform(0.0, r_max)]
            for _ in range(n)]


def edt_costmap(occupied, power=10):
    """create_costmap.py:15-28: distance to nearest obstacle -> min-max normalise -> (1-d)**power."""
    from scipy.ndimage import distance_transform_edt
    d = distance_transform_edt(~occupied).astype(np.float64)
    lo, hi = d.min(), d.max()
    dn = (d - lo) / (hi - lo) if hi > lo else np.zeros_like(d)
    return ((1.0 - dn) ** power).astype(np.float32)


def disc_costmap(size, half_width, obstacles, inflate=0.5, power=10):
    """Binary disc raster (MPPI_OO_current.py:291-296: r + r_robot(0.3) + 0.2) -> edt_costmap."""
    x = np.linspace(-half_width, half_width, size)
    X, Y = np.meshgrid(x, x)
    occ = np.zeros((size, size), bool)
    for ox, oy, r in obstacles:
        rr = r + inflate
        # bounding box only
        i0 = max(0, int((ox - rr + half_width) / (2 * half_width) * (size - 1)) - 1)
        i1 = min(size, int((ox + rr + half_width) / (2 * half_width) * (size - 1)) + 2)
        j0 = max(0, int((oy - rr + half_width) / (2 * half_width) * (size - 1)) - 1)
        j1 = min(size, int((oy + rr + half_width) / (2 * half_width) * (size - 1)) + 2)
        sub = (X[j0:j1, i0:i1] - ox) ** 2 + (Y[j0:j1, i0:i1] - oy) ** 2 <= rr ** 2
        occ[j0:j1, i0:i1] |= sub
    return edt_costmap(occ, power)


def surface_obstacles_costmap(costmap_size, half_width, obstacles, origin, r_robot, power=20):
    """Surface.create_obstacles_costmap (MPPI_isaac.py:361-378) with scipy's EDT in place of cv2.

    Frame swap x_local = y - y0, y_local = x - x0 and radius r/2 + r_robot + 0.1, as the reference.
    """
    x = np.linspace(-half_width, half_width, costmap_size)
    X, Y = np.meshgrid(x, x)
    occ = np.zeros((costmap_size, costmap_size), bool)
    x0, y0 = origin
    for xg, yg, r in obstacles:
        xl = yg - y0
        yl = xg - x0
        tr = r / 2 + r_robot + 0.1
        occ |= (X - xl) ** 2 + (Y - yl) ** 2 <= tr ** 2
    return edt_costmap(occ, power)


def scene_c3():
    """Configs C1-C4: 1500^2 DEM @0.1 m (half-width 75), 750^2 costmap @0.2 m."""
    Z = crater_dem(1500, 75.0)
    cm = disc_costmap(750, 75.0, random_obstacles())
    return Z, 75.0, cm


def _fbm_factors(grid, half_width, seed=7, octaves=5, amp=0.3, base_wavelength=8.0):
    """Seeded band-limited fBm (random sinusoid octaves) as rank-1 factors (row, column) pairs.

    sin(kx x + ky y + ph) = cos(ky y) sin(kx x + ph) + sin(ky y) cos(kx x + ph).
    """
    rng = np.random.RandomState(seed)
    x = np.linspace(-half_width, half_width, grid, dtype=np.float32)
    rows, cols = [], []
    for o in range(octaves):
        lam = base_wavelength / (2 ** o)
        a = np.float32(amp / (2 ** o))
        for _ in range(3):
            th = rng.uniform(0, np.pi)
            ph = rng.uniform(0, 2 * np.pi)
            kx = np.float32(2 * np.pi / lam * np.cos(th))
            ky = np.float32(2 * np.pi / lam * np.sin(th))
            ax = kx * x + np.float32(ph)
            by = ky * x
            rows += [a * np.cos(by), a * np.sin(by)]
            cols += [np.sin(ax), np.cos(ax)]
    return rows, cols


def _crater_factors(grid_size, half_width, bumps=BUMPS_9, scale=1.0):
    """The crater formula of MPPI_isaac.py:318-320 with each gaussian split as exp(-dy^2/2w^2) x exp(-dx^2/2w^2)."""
    x = np.linspace(-half_width, half_width, grid_size)
    rows, cols = [], []
    for (cx, cy), h, w in bumps:
        cx, cy, w = cx * scale, cy * scale, w * scale
        for amp, ww in ((h - 0.5, w), (-(h + 0.5), w / 2)):
            rows.append((amp * np.exp(-(x - cy) ** 2 / (2 * ww ** 2))).astype(np.float32))
            cols.append(np.exp(-(x - cx) ** 2 / (2 * ww ** 2)).astype(np.float32))
    return rows, cols


def fbm(grid, half_width, seed=7, octaves=5, amp=0.3, base_wavelength=8.0):
    """Seeded band-limited fBm (sum of random sinusoid octaves), for C5 roughness."""
    rows, cols = _fbm_factors(grid, half_width, seed, octaves, amp, base_wavelength)
    return np.stack(rows, 1) @ np.stack(cols, 0)


def scene_c5():
    """Config C5: 8192^2 DEM @0.025 m (half-width 102.4), craters x2 in size + fBm; 1024^2 costmap.

    The terrain is a sum of 48 separable terms (18 crater gaussians, 30 fBm sinusoids), built as
    one float32 (8192 x 48) @ (48 x 8192) product, so the tile takes a second, not ~30 s.
    """
    r1, c1 = _crater_factors(8192, 102.4, scale=4.0 / 1.0 * 0.5)
    r2, c2 = _fbm_factors(8192, 102.4)
    Z = np.stack(r1 + r2, 1) @ np.stack(c1 + c2, 0)
    cm = disc_costmap(1024, 102.4, random_obstacles(extent=90.0))
    return Z.astype(np.float32), 102.4, cm
