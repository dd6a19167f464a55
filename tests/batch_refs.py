"""Closed-loop references for the batched episodes (tests/test_batch_host.py, tests/test_gpu_batch.py).

The advance rule of the issue / DESIGN.md §3.7 is written out here on its own (not through
mppi_amd.batch.advance_state, which the CPU test checks against it):

  reference A  the loop over oracle.mppi_ref.mppi_step (CPU, no engine)
  reference B  the same loop over a fresh Engine(seed=seed_e).step (GPU)

Both pass the RAW row-0 heading on (oracle State / make_state normalise it with np.linalg.norm),
use step index = loop count, and return what a batch reports: log rows [n, 8], the final state, the
final nominal sequence, the step count and `reached`.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from oracle import mppi_ref as R

F32 = np.float32
RUN = dict(sigma_base=0.4, sigma_div=1.0, goal_tol=0.5)
ISAAC = dict(sigma_base=0.25, sigma_div=3.0, goal_tol=0.5)
START = (-60.0, -5.0)

# The main case of the issue: (start, goal, seed, K); heading (1, 0, 0), H = 20, run() policy, 40 steps.
MAIN = [
    (START, (-59.3, -4.9), 7, 256),
    (START, (-59.2, -5.2), 8, 300),
    ((10.0, 12.0), (10.75, 12.0), 9, 256),
    (START, (-59.6, -4.8), 3, 256),      # starts inside the tolerance: no step
    (START, (65.0, 10.0), 1, 256),       # far goal: runs to the cap
]


def start_state(start, goal, heading=(1.0, 0.0, 0.0), s1=0.25, s2=0.25):
    return dict(x=F32(start[0]), y=F32(start[1]), heading=np.asarray(heading, np.float64),
                wl=F32(0.0), wr=F32(0.0), gx=F32(goal[0]), gy=F32(goal[1]), s1=F32(s1), s2=F32(s2))


def active(st, pol):
    tol = F32(pol["goal_tol"])
    # inside the tolerance on both axes ends the loop; a NaN coordinate is never inside
    return not bool(np.abs(F32(st["x"] - st["gx"])) <= tol and np.abs(F32(st["y"] - st["gy"])) <= tol)


def rule(st, traj0, hv0, v, w, r, pol):
    """(next state with the raw heading, log row) by the advance rule, float32 / float64 written out."""
    base, div = F32(pol["sigma_base"]), F32(pol["sigma_div"])
    traj0 = np.asarray(traj0, F32)
    hv = np.asarray(hv0, F32)
    v, w, r = F32(v), F32(w), F32(r)
    h0, h1, h2 = np.float64(hv[0]), np.float64(hv[1]), np.float64(hv[2])
    n = np.sqrt((h0 * h0 + h1 * h1) + h2 * h2)
    hn = np.array([F32(h0 / n), F32(h1 / n), F32(h2 / n)], F32)
    ww = F32(F32(w * w) / div)
    half = F32(F32(w * r) / F32(2.0))
    new = dict(x=traj0[0], y=traj0[1], heading=hv.astype(np.float64), heading_n=hn,
               wl=F32(v - half), wr=F32(v + half), gx=st["gx"], gy=st["gy"],
               s1=max(base, F32(base - ww)), s2=max(base, F32(base + ww)))
    row = np.array([traj0[0], traj0[1], traj0[2], hn[0], hn[1], hn[2], v, w], F32)
    return new, row


def _result(rows, st, u1, u2, steps, pol):
    hn = st.get("heading_n")
    if hn is None:   # no step taken: the start heading as given
        hn = np.asarray(st["heading"], F32)
    final = np.array([st["x"], st["y"], hn[0], hn[1], hn[2], st["wl"], st["wr"], st["gx"], st["gy"],
                      st["s1"], st["s2"]], F32)
    return dict(rows=np.asarray(rows, F32).reshape(-1, 8), final=final, u1=np.asarray(u1, F32),
                u2=np.asarray(u2, F32), steps=steps, reached=not active(st, pol))


def oracle_loop(K, H, scene, st, seed, n_steps, proj="3d", pol=RUN, params=None):
    """Reference A."""
    p = dataclasses.replace(params or R.Params(), K=K, H=H, seed=seed)
    u1 = np.zeros(H, F32)
    u2 = np.zeros(H, F32)
    rows = []
    i = 0
    while i < n_steps and active(st, pol):
        S = R.State(x=float(st["x"]), y=float(st["y"]), heading=np.asarray(st["heading"], np.float64),
                    left_wheel_speed=float(st["wl"]), right_wheel_speed=float(st["wr"]),
                    goal_x=float(st["gx"]), goal_y=float(st["gy"]), std_dev_u1=float(st["s1"]),
                    std_dev_u2=float(st["s2"]))
        o = R.mppi_step(p, scene, S, u1, u2, i, proj)
        u1, u2 = o["u1_opt"], o["u2_opt"]
        st, row = rule(st, o["traj_sim"][0], o["hv_sim"][0], o["v_opt"][0], o["w_opt"][0], p.robot_radius, pol)
        rows.append(row)
        i += 1
    return _result(rows, st, u1, u2, i, pol)


def engine_loop(K, H, Z, hw, cm, st, seed, n_steps, proj="3d", pol=RUN, make_engine=None):
    """Reference B: a fresh Engine at its default options, stepped from the host.  make_engine(seed), if
    given, builds it instead, scene bound (other parameters or grid geometry; Z, hw, cm are then unused)."""
    from mppi_amd import _lib
    eng = make_engine(seed) if make_engine else _lib.Engine(_lib.make_params(K, H, seed=seed), 0)
    try:
        if not make_engine:
            eng.set_dem(Z, hw)
            eng.set_costmap(cm, hw)
        r = float(eng.params.robot_radius)
        rows = []
        i = 0
        while i < n_steps and active(st, pol):
            eng.set_state(_lib.make_state(st["x"], st["y"], st["heading"], st["wl"], st["wr"], st["gx"], st["gy"],
                                          st["s1"], st["s2"]))
            o = eng.step(proj, i)
            st, row = rule(st, o["traj_sim"][0], o["heading_sim"][0], o["lin_vel"][0], o["ang_vel"][0], r, pol)
            rows.append(row)
            i += 1
        u1, u2 = eng.get_nominal()
    finally:
        eng.close()
    return _result(rows, st, u1, u2, i, pol)


@functools.lru_cache(maxsize=None)
def oracle_main(e, n_steps=40, H=20):
    """Reference A of episode e of the main case (computed once per session)."""
    from helpers import c3_scene, oracle_scene
    start, goal, seed, K = MAIN[e]
    return oracle_loop(K, H, oracle_scene(*c3_scene()), start_state(start, goal), seed, n_steps)
