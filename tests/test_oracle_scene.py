"""Host: the oracle's Scene on a DEM that is neither square nor centred, against the cell rule of
include/mppi.h (mppi_set_dem): column trunc((x - x_min) / res), row -trunc((y + y_min) / res), clamped.

3 rows x 5 columns at res 0.5 with x_min = -1, y_min = -2: column 0 starts at x = -1, row 0 lies at
y = 2, the map spans x in [-1, 1.5] and y in (0.5, 2.5).  Z[r, c] = 5 r + c names the cell.  Every
coordinate is a multiple of 1/8, so each quotient below is exact and the expected cells are plain
arithmetic done by hand.
"""
import numpy as np

import helpers as hp
from oracle import mppi_ref as R

F32 = np.float32
ROWS, COLS, RES, X_MIN, Y_MIN = 3, 5, 0.5, -1.0, -2.0

# x -> (x + 1) / 0.5 -> trunc (dem_cell keeps it within [-1, COLS]) -> clamped column
XS = [(-1.0, 0, 0),      # 0.0   the left edge itself
      (0.25, 2, 2),      # 2.5
      (1.375, 4, 4),     # 4.75  last column
      (1.625, 5, 4),     # 5.25  right of the map: clamped
      (40.0, 5, 4),      # 82    far right: the index saturates at COLS before the clamp
      (-1.25, 0, 0),     # -0.5  left of the map but trunc(-0.5) = 0 (the reference's trunc quirk)
      (-1.75, -1, 0),    # -1.5  left of the map: clamped
      (-40.0, -1, 0)]    # -78   far left: saturates at -1
# y -> (y - 2) / 0.5 -> minus trunc (within [-1, ROWS]) -> clamped row
YS = [(2.0, 0, 0),       # 0.0   row 0's own line
      (1.375, 1, 1),     # -1.25
      (0.875, 2, 2),     # -2.25 last row
      (0.375, 3, 2),     # -3.25 below the map: clamped
      (-40.0, 3, 2),     # -84   far below: saturates at ROWS
      (2.25, 0, 0),      # 0.5   above the map but trunc(0.5) = 0
      (2.625, -1, 0),    # 1.25  above the map: clamped
      (40.0, -1, 0)]     # 76    far above: saturates at -1


def _scene():
    Z = np.arange(ROWS * COLS, dtype=F32).reshape(ROWS, COLS)
    return hp.scene_for(Z, np.zeros((1, 1), F32), half_width=7.0, resolution=RES, x_min=X_MIN, y_min=Y_MIN)


def test_scene_defaults_are_the_centred_square():
    sc = R.Scene(np.zeros((6, 6), F32), 1.5, np.zeros((3, 3), F32))
    assert (sc.x_min, sc.y_min, sc.res, sc.res_c, sc.hw) == (F32(-1.5), F32(-1.5), F32(0.5), F32(1.0), F32(1.5))
    assert (sc.rows, sc.grid, sc.size) == (6, 6, 3)
    same = hp.scene_for(np.zeros((6, 6), F32), np.zeros((3, 3), F32), 1.5)
    assert (same.x_min, same.y_min, same.res, same.res_c, same.hw) == (sc.x_min, sc.y_min, sc.res, sc.res_c, sc.hw)


def test_cells_of_a_non_square_off_centre_dem():
    sc = _scene()
    assert (sc.rows, sc.grid) == (ROWS, COLS) and (sc.x_min, sc.y_min, sc.res) == (F32(X_MIN), F32(Y_MIN), F32(RES))
    assert sc.hw == F32(7.0) and sc.res_c == F32(14.0)    # the costmap keeps its own half width
    for x, col_raw, col in XS:
        for y, row_raw, row in YS:
            xa, ya = np.array([x], F32), np.array([y], F32)
            i, j = R.dem_cell(sc, xa, ya)
            assert (int(i[0]), int(j[0])) == (col_raw, row_raw), (x, y, i, j)
            assert R.dem_at(sc, j, i)[0] == F32(5 * row + col), (x, y)
            q = R.get_corners_heights(sc, xa, ya)
            r1, c1 = min(max(row_raw + 1, 0), ROWS - 1), min(max(col_raw + 1, 0), COLS - 1)
            want = (5 * row + col, 5 * row + c1, 5 * r1 + col, 5 * r1 + c1)
            assert tuple(float(v[0]) for v in q) == tuple(float(v) for v in want), (x, y, q, want)


def test_transposed_shape_is_another_scene():
    """rows and grid are not interchangeable: the same points on the 5 x 3 map."""
    Z = np.arange(ROWS * COLS, dtype=F32).reshape(COLS, ROWS)
    sc = hp.scene_for(Z, np.zeros((1, 1), F32), half_width=7.0, resolution=RES, x_min=X_MIN, y_min=Y_MIN)
    i, j = R.dem_cell(sc, np.array([40.0, 0.25], F32), np.array([-40.0, -0.125], F32))
    assert i.tolist() == [3, 2] and j.tolist() == [5, 4]       # saturate at grid = 3 and rows = 5
    assert R.dem_at(sc, j, i).tolist() == [14.0, 14.0]         # Z[4, 2]
