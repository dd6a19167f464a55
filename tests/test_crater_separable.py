"""CPU: mppi_amd.scene.crater_dem_separable, the numpy float64 restatement of the on-device crater-field
builder, against the reference's own Surface.create_surface output
(tests/golden/crater_fields.npz), and the CraterField plumbing of the controller's batch set-up.

Measured here: 0 differing cells in every fixture case (the float64 sums differ from the reference's by
at most 3.6e-14, so a cell differs only when its value lies that close to a float32 rounding boundary).
"""
import functools
import types

import numpy as np
import pytest

from crater_helpers import CASE_IDS, GOLDEN, assert_dem_close, crater_cases
from mppi_amd import controller, scene


@pytest.mark.parametrize("case", range(4), ids=CASE_IDS)
def test_separable_matches_the_reference(case):
    grid, hw, craters, ref = crater_cases()[case]
    got = scene.crater_dem_separable(grid, hw, craters)
    assert_dem_close(got, ref, f"separable {CASE_IDS[case]}")


def test_no_crater_gives_zeros_or_the_base():
    Z = scene.crater_dem_separable(17, 0.85, [])
    assert Z.dtype == np.float32 and Z.shape == (17, 17) and not Z.any()
    base = (np.arange(17 * 17, dtype=np.float32) * np.float32(1e-3)).reshape(17, 17)
    assert np.array_equal(scene.crater_dem_separable(17, 0.85, np.zeros((0, 4)), base=base), base)


def test_base_is_added_before_the_single_rounding():
    grid, hw, craters, _ = crater_cases()[2]
    Z64 = np.load(GOLDEN)["Z_2"]   # the reference's float64 field
    base = (np.float32(1e-3) * np.arange(grid * grid, dtype=np.float32)).reshape(grid, grid)
    once = (Z64 + base.astype(np.float64)).astype(np.float32)
    twice = Z64.astype(np.float32) + base
    # the pattern tells the two apart: rounding the craters first moves far more cells than the rule allows
    assert np.count_nonzero(once != twice) > 0.01 * once.size
    assert_dem_close(scene.crater_dem_separable(grid, hw, craters, base=base), once, "with base")


def test_both_crater_list_forms_are_accepted():
    grid, hw, craters, _ = crater_cases()[1]
    nested = [((float(r[0]), float(r[1])), float(r[2]), float(r[3])) for r in craters]
    a = scene.crater_dem_separable(grid, hw, craters)
    assert np.array_equal(a, scene.crater_dem_separable(grid, hw, nested))
    assert np.array_equal(a, scene.crater_dem_separable(grid, hw, [tuple(r) for r in craters]))
    f = scene.CraterField(nested)
    assert len(f) == 3 and np.array_equal(f.rows, craters) and np.array_equal(f.dem(grid, hw), a)
    assert np.array_equal(scene.crater_rows(scene.BUMPS_9)[1], [-0.57, -0.05, 4.39, 11.52])
    with pytest.raises(ValueError, match="crater 0"):
        scene.crater_rows([(1.0, 2.0, 3.0)])
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        scene.crater_rows(np.zeros((2, 3)))


class _StubBatch:
    def __init__(self, engine, episodes):
        self.calls = []

    def build_dem(self, slot, bumps, half_width, base=None, copy_out=False, variant="mfma"):
        self.calls.append(("build_dem", slot, bumps, half_width, base))

    def set_dem(self, slot, Z):
        self.calls.append(("set_dem", slot, Z))

    def set_episode(self, *a):
        self.calls.append(("set_episode",) + a)

    def close(self):
        pass


def test_open_batch_builds_crater_fields_and_uploads_arrays(monkeypatch):
    monkeypatch.setattr(controller._lib, "Batch", _StubBatch)
    C = controller.MPPI_Controller
    me = types.SimpleNamespace(seed=1, number_of_trajectories=256, engine=types.SimpleNamespace(dem_shape=(8, 8)),
                               surface=types.SimpleNamespace(half_width=4.0))
    me._fill_dem_slot = functools.partial(C._fill_dem_slot, me)
    base = np.ones((8, 8), np.float32)
    field = scene.CraterField([((0.5, -0.5), 2.0, 1.0)], base=base)
    flat = np.arange(64, dtype=np.float64)
    states = [object(), object()]
    batch = C._open_batch(me, 2, lambda: states, None, None, None, [field, flat], None, [0, 1], None, None)
    calls = [c for c in batch.calls if c[0] != "set_episode"]
    assert calls[0][:2] == ("build_dem", 0) and calls[0][2] is field and calls[0][3] == 4.0 and calls[0][4] is field.base
    assert calls[1][:2] == ("set_dem", 1) and calls[1][2].shape == (8, 8) and calls[1][2].dtype == np.float32
    assert np.array_equal(calls[1][2].ravel(), flat.astype(np.float32))
    assert [c[5] for c in batch.calls if c[0] == "set_episode"] == [0, 1]   # each episode's DEM slot
