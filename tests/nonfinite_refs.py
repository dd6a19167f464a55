"""Shared by the non-finite tests: dead sets, patched scenes, NaN-aware equality.

Scenes.  A flat-ish 400 x 400 DEM at 0.1 m (x, y in +-20 m) with a smooth finite relief, the rover at
the origin heading +x, the goal far ahead.  `patched_dem(kind, x_from)` replaces every cell with
x >= x_from by NaN, +inf, or a checkerboard of +-3e38 whose differences overflow.  A trajectory
that drives into the patch gets a NaN normal, then a NaN position and a cost that is not finite; one
that stays short of it never reads a patched cell.  `chosen_controls(dead, H)` gives finite controls
that drive exactly the trajectories of `dead` into the patch: those run at 0.7 .. 1.0 of full speed,
the others creep at 0.02 .. 0.12, both with a little steering so that the costs differ.  The tests
assert on the oracle's costs that the dead set is the intended one before they look at the engine.
"""
from __future__ import annotations

import numpy as np

from oracle import mppi_ref as R

F32 = np.float32
LEAF = R.LEAF
POS_NAN = np.array([0x7FC00000], np.uint32).view(F32)[0]
NEG_NAN = np.array([0xFFC00000], np.uint32).view(F32)[0]
PATTERNS = ("lane", "line", "half", "leaf", "all-but-one", "all")
PATCH_KINDS = ("nan", "inf", "3e38")
HW = 20.0
GRID = 400
X_FROM = {24: 0.45, 100: 2.5}     # where the patch begins, per horizon: past the creeping trajectories' reach


def dead_set(pattern, K):
    """bool[K]: the trajectories a pattern kills."""
    k = np.arange(K)
    lane, leaf = k % LEAF, k // LEAF
    last = (K - 1) // LEAF
    if pattern == "lane":          # one lane in every leaf, a different line in each
        return lane == (37 + 32 * leaf) % LEAF
    if pattern == "line":          # the 32-line 3 of the last leaf that has one
        full = last if K % LEAF == 0 or K % LEAF > 128 else max(last - 1, 0)
        return (leaf == full) & (lane // 32 == 3)
    if pattern == "half":          # the upper half of leaf 0
        return (leaf == 0) & (lane >= 128)
    if pattern == "leaf":          # the whole last leaf
        return leaf == last
    if pattern == "all-but-one":   # leaf 0 keeps lane 201 only
        return (leaf == 0) & (lane != 201)
    if pattern == "all":
        return np.ones(K, bool)
    raise ValueError(pattern)


def base_dem():
    xs = (np.arange(GRID) + 0.5) * (2.0 * HW / GRID) - HW
    X, Y = np.meshgrid(xs, -xs)
    return (0.3 * np.sin(0.7 * X) * np.cos(0.5 * Y) + 0.02 * X).astype(F32)


def patched_dem(kind, x_from, y_from=None):
    """base_dem with the cells at x >= x_from (and y >= y_from, when given) replaced."""
    Z = base_dem()
    xs = (np.arange(GRID) + 0.5) * (2.0 * HW / GRID) - HW
    X, Y = np.meshgrid(xs, -xs)
    sel = X >= x_from
    if y_from is not None:
        sel &= Y >= y_from
    if kind == "nan":
        Z[sel] = POS_NAN
    elif kind == "inf":
        Z[sel] = F32(np.inf)
    elif kind == "3e38":
        ii, jj = np.meshgrid(np.arange(GRID), np.arange(GRID))
        Z[sel] = np.where((ii + jj) % 2 == 0, F32(3e38), F32(-3e38))[sel]
    else:
        raise ValueError(kind)
    return Z


def flat_costmap(size=100):
    return np.zeros((size, size), F32)


def chosen_controls(dead, H, seed=0):
    """Finite controls [K, H] x 2: the trajectories of `dead` drive into the patch at X_FROM[H]."""
    rng = np.random.RandomState(seed)
    K = dead.size
    base = np.where(dead, rng.uniform(0.7, 1.0, K), rng.uniform(0.02, 0.12, K))
    steer = np.where(dead, rng.uniform(-0.1, 0.1, K), rng.uniform(-0.01, 0.01, K))
    u1 = np.clip(base - steer, -1.0, 1.0)[:, None] * np.ones((1, H))
    u2 = np.clip(base + steer, -1.0, 1.0)[:, None] * np.ones((1, H))
    return u1.astype(F32), u2.astype(F32)


# ------------------------------------------------------------------ equality with NaN == NaN
def same_bits_or_nan(got, want):
    """Elementwise: both NaN (any sign or payload), or the same bit pattern."""
    g = np.ascontiguousarray(got)
    w = np.ascontiguousarray(want, g.dtype)
    assert g.shape == w.shape, (g.shape, w.shape)
    iv = np.uint32 if g.dtype == np.float32 else np.uint64
    gn, wn = np.isnan(g), np.isnan(w)
    return (gn & wn) | (~gn & ~wn & (g.view(iv) == w.view(iv)))


def nan_report(name, got, want, n=5):
    ok = same_bits_or_nan(got, want).reshape(-1)
    bad = np.nonzero(~ok)[0][:n]
    g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    return f"{name}: {int((~ok).sum())}/{ok.size} differ; first {bad.tolist()} got {g[bad].tolist()} want {w[bad].tolist()}"


def assert_same(name, got, want):
    assert same_bits_or_nan(got, want).all(), nan_report(name, got, want)


def specified_prefix(a):
    """bool mask like a [K, H, C] (or [H, C]): the elements of each trajectory, in row-major order,
    before its first element that is not finite (D13: a dumped array is specified up to there)."""
    x = np.asarray(a)
    flat = x.reshape(x.shape[0], -1) if x.ndim == 3 else x.reshape(1, -1)
    bad = ~np.isfinite(flat)
    return (np.cumsum(bad, axis=1) == 0).reshape(x.shape)
