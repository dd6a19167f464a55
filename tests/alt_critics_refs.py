"""References for the critic set (include/mppi.h mppi_critics; tests/test_alt_critics_host.py,
tests/test_gpu_alt_critics.py, tests/test_gpu_batch_alt_critics.py).

oracle.mppi_ref.rollout_costs calls `critics` by module name, so a test swaps it for a wrapper with
pytest's monkeypatch (`use`); everything else of the oracle's step runs as it is.

  body slope   the oracle's own critics called with lw = rw = traj: _avoid_slope
               (critics_warp.py:131-166) is the wheel form with both wheels on the body path.
  orientation  _path_orientation_critic (:44-82), float32 numpy below.  With a weight != 0 the cost
               is summed in the menu's order (:324-329): w_orientation po, + w_path pf, + w_slope
               slope, + w_speed sp, + w_obstacle ob.  The four values come from the oracle's function
               with one weight 1 and the others 0 (1 * t + 0 * .. is t for finite values).  With
               weight 0 the wrapper is the oracle's function alone: today's bits.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import batch_refs as B
import helpers as hp
from oracle import mppi_ref as R

F32 = np.float32
ORACLE_CRITICS = R.critics          # (taken before any test patches the module)
WEIGHTS = ("w_path", "w_slope", "w_speed", "w_obstacle")
DEFAULT = dict(slope="wheels", w_orientation=0.0)

# the single-step case and the closed-loop case of the issue
K1, H1, SEED1 = 256, 20, 5
SEED_LOOP, STEPS_LOOP = 7, 8
FAR = (65.0, 10.0)
BACK = (-1.0, 0.0, 0.0)             # heading away from the goal: every rollout has po != 0
SIDE = (0.0, 1.0, 0.0)


def orientation(st: R.State, traj):
    """po [K] of rollouts traj [K, H, 3] (H >= 2) for the robot and goal of st."""
    x, y = F32(st.x), F32(st.y)
    xd = F32(st.goal_x) - x
    yd = F32(st.goal_y) - y
    H = traj.shape[1]
    x2 = traj[:, H - 1, 0] - traj[:, H - 2, 0]
    y2 = traj[:, H - 1, 1] - traj[:, H - 2, 1]
    s = (xd * x2) + (yd * y2)
    den = np.abs(xd) + np.abs(yd)
    if den == 0:                    # DEFINED: the reference divides 0 by 0
        return np.zeros(traj.shape[0], F32)
    return np.where(s <= 0, (-s) / den, F32(0.0)).astype(F32)


def terms(p, sc, st, traj, lw, rw, v):
    """[K, 4] unweighted path, slope, speed, obstacle values from the oracle's function."""
    return np.stack([ORACLE_CRITICS(dataclasses.replace(p, **{w: (1.0 if w == one else 0.0) for w in WEIGHTS}),
                                    sc, st, traj, lw, rw, v) for one in WEIGHTS], -1).astype(F32)


def make_critics(slope="wheels", w_orientation=0.0):
    """A drop-in for oracle.mppi_ref.critics under the given critic set."""
    assert slope in ("wheels", "body")
    wo = F32(w_orientation)

    def critics(p, sc, st, traj, lw, rw, v):
        if slope == "body":
            lw = rw = traj
        if wo == 0:
            return ORACLE_CRITICS(p, sc, st, traj, lw, rw, v)
        t = terms(p, sc, st, traj, lw, rw, v)
        c = wo * orientation(st, traj)
        for i, w in enumerate(WEIGHTS):
            c = c + p.f(w) * t[:, i]
        return c.astype(F32)

    return critics


def use(monkeypatch, slope="wheels", w_orientation=0.0):
    """The oracle computes with this critic set until the test ends."""
    monkeypatch.setattr(R, "critics", make_critics(slope, w_orientation))


def recombine(t5, weights, w_orientation):
    """Costs [K] from terms [K, 5] (COST_TERMS5 order) in the menu's order, float32."""
    t5 = np.asarray(t5, F32)
    w = [F32(x) for x in weights]
    wo = F32(w_orientation)
    c = w[0] * t5[:, 0]
    if wo != 0:
        c = wo * t5[:, 4] + c
    for i in (1, 2, 3):
        c = c + w[i] * t5[:, i]
    return c.astype(F32)


def single_step(proj, crit, heading=(1.0, 0.0, 0.0), K=K1, H=H1, seed=SEED1, step=0, goal=FAR):
    """The oracle's step of the issue's single-step case under critic set `crit` (no monkeypatch
    needed: the module attribute is swapped for the call only)."""
    st = hp.oracle_state(heading=heading, wl=0.3, wr=0.5, goal=goal)
    sc = hp.oracle_scene(*hp.c3_scene())
    p = R.Params(K=K, H=H, seed=seed)
    saved = R.critics
    R.critics = make_critics(**crit)
    try:
        return R.mppi_step(p, sc, st, np.zeros(H, F32), np.zeros(H, F32), step, proj=proj), st
    finally:
        R.critics = saved


def loop(proj, crit, heading=(1.0, 0.0, 0.0), seed=SEED_LOOP, steps=STEPS_LOOP):
    """Reference A of the closed-loop case under `crit`: batch_refs.oracle_loop, K = 256, H = 20."""
    saved = R.critics
    R.critics = make_critics(**crit)
    try:
        return B.oracle_loop(K1, H1, hp.oracle_scene(*hp.c3_scene()), B.start_state(B.START, FAR, heading), seed, steps,
                             proj)
    finally:
        R.critics = saved


def engine_loop(proj, crit, heading=(1.0, 0.0, 0.0), seed=SEED_LOOP, steps=STEPS_LOOP):
    """Reference B: a fresh engine with set_critics, stepped from the host."""
    from mppi_amd import _lib
    Z, hw, cm = hp.c3_scene()

    def make(seed_):
        eng = _lib.Engine(_lib.make_params(K1, H1, seed=seed_), 0)
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        eng.set_critics(**crit)
        return eng

    return B.engine_loop(K1, H1, Z, hw, cm, B.start_state(B.START, FAR, heading), seed, steps, proj, make_engine=make)


def rows_changed(a, b):
    """Log rows of two runs of equal length that are not bitwise equal."""
    assert a["rows"].shape == b["rows"].shape
    return int((a["rows"].view(np.uint32) != b["rows"].view(np.uint32)).any(axis=1).sum())
