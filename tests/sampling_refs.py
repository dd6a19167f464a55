"""References for sampling plans (include/mppi.h mppi_sampling; tests/test_sampling_*.py,
tests/test_gpu_sampling*.py).

The expected step for a plan needs no change to the oracle: base normals from oracle.dmath.noise at
the plan's source indices, mppi_amd.sampling.apply_plan, oracle.mppi_ref.sample_controls, then
oracle.mppi_ref.mppi_step(injected=(u1, u2)).  Everything is compared bitwise.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import batch_refs as B
import helpers as hp
from mppi_amd import sampling as S
from oracle import dmath
from oracle import mppi_ref as R

F32 = np.float32
DEFAULT = dict(antithetic=False, nominal=False, beta=0.0)
NOMINAL = dict(antithetic=False, nominal=True, beta=0.0)
ANTI = dict(antithetic=True, nominal=False, beta=0.0)
BETA = dict(antithetic=False, nominal=False, beta=0.7)
NOM_ANTI = dict(antithetic=True, nominal=True, beta=0.0)
ALL = dict(antithetic=True, nominal=True, beta=0.7)
PLANS = dict(nominal=NOMINAL, antithetic=ANTI, beta=BETA, combined=ALL)
SHAPES = [(300, 5), (256, 20)]      # two ragged leaves and an odd H; C1, the server's plan
FAR = (65.0, 10.0)
OUT_KEYS = (("u1_opt", "u1_opt"), ("u2_opt", "u2_opt"), ("lin_vel", "v_opt"), ("ang_vel", "w_opt"),
            ("traj_sim", "traj_sim"), ("heading_sim", "hv_sim"))


def controls(p: R.Params, st: R.State, u_nom1, u_nom2, step, plan, k_begin=0, k_count=None):
    """(u1, u2) [k_count, H]: the sampled controls of global trajectories k_begin .. under `plan`."""
    k = np.arange(k_begin, k_begin + (p.K if k_count is None else k_count), dtype=np.int64)
    src, _, _ = S.plan_sources(k, plan)
    z1, z2 = dmath.noise(p.seed, step, src, p.H)
    e1, e2 = S.apply_plan(z1, z2, k, plan)
    return R.sample_controls(p, st, u_nom1, u_nom2, e1, e2)


def expected_step(p, sc, st, u_nom1, u_nom2, step, plan, proj="3d"):
    """The oracle's step under `plan`, with the sampled controls it rolled out as out["u1"], out["u2"]."""
    u1, u2 = controls(p, st, u_nom1, u_nom2, step, plan)
    out = R.mppi_step(p, sc, st, u_nom1, u_nom2, step, proj, injected=(u1, u2))
    out["u1"], out["u2"] = u1, u2
    return out


def same_step(got, costs, want, tag):
    """An engine step's outputs and costs against expected_step's, bitwise."""
    for a, b in OUT_KEYS:
        g, w = np.asarray(got[a], F32), np.asarray(want[b], F32)
        assert g.shape == w.shape, (tag, a, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{tag}: " + hp.mismatch_report(a, g, w)
    c, w = np.asarray(costs, F32), np.asarray(want["cost"], F32)
    assert np.array_equal(c.view(np.uint32), w.view(np.uint32)), f"{tag}: " + hp.mismatch_report("cost", c, w)


def next_state(st: R.State, out, p: R.Params, pol=B.RUN):
    """The closed loop's next oracle state from a step's outputs (batch_refs.rule; engine or oracle keys)."""
    d = dict(x=F32(st.x), y=F32(st.y), gx=F32(st.goal_x), gy=F32(st.goal_y))
    hv = out["heading_sim"] if "heading_sim" in out else out["hv_sim"]
    v = out["lin_vel"] if "lin_vel" in out else out["v_opt"]
    w = out["ang_vel"] if "ang_vel" in out else out["w_opt"]
    new, _ = B.rule(d, out["traj_sim"][0], hv[0], v[0], w[0], p.robot_radius, pol)
    return R.State(x=float(new["x"]), y=float(new["y"]), heading=np.asarray(new["heading"], np.float64),
                   left_wheel_speed=float(new["wl"]), right_wheel_speed=float(new["wr"]), goal_x=st.goal_x,
                   goal_y=st.goal_y, std_dev_u1=float(new["s1"]), std_dev_u2=float(new["s2"]))


def closed_loop(K, H, seed, plan, n_steps, proj="3d", st=None, plans=None):
    """n_steps expected steps in closed loop from u_nom = 0: a list of (state, u_nom1, u_nom2, out).
    plans: a plan per step (a switching schedule) instead of `plan` for all."""
    sc = hp.oracle_scene(*hp.c3_scene())
    p = R.Params(K=K, H=H, seed=seed)
    st = st or hp.oracle_state(wl=0.3, wr=0.5, goal=FAR)
    u1, u2 = np.zeros(H, F32), np.zeros(H, F32)
    steps = []
    for i in range(n_steps):
        out = expected_step(p, sc, st, u1, u2, i, plans[i] if plans else plan, proj)
        steps.append((st, u1, u2, out))
        u1, u2 = out["u1_opt"], out["u2_opt"]
        st = next_state(st, out, p)
    return steps


def oracle_loop(K, H, st, seed, n_steps, plan, proj="3d", pol=B.RUN, params=None):
    """batch_refs.oracle_loop (reference A of a batch episode) under a sampling plan."""
    sc = hp.oracle_scene(*hp.c3_scene())
    p = dataclasses.replace(params or R.Params(), K=K, H=H, seed=seed)
    u1, u2 = np.zeros(H, F32), np.zeros(H, F32)
    rows, i = [], 0
    while i < n_steps and B.active(st, pol):
        S_ = R.State(x=float(st["x"]), y=float(st["y"]), heading=np.asarray(st["heading"], np.float64),
                     left_wheel_speed=float(st["wl"]), right_wheel_speed=float(st["wr"]), goal_x=float(st["gx"]),
                     goal_y=float(st["gy"]), std_dev_u1=float(st["s1"]), std_dev_u2=float(st["s2"]))
        o = expected_step(p, sc, S_, u1, u2, i, plan, proj)
        u1, u2 = o["u1_opt"], o["u2_opt"]
        st, row = B.rule(st, o["traj_sim"][0], o["hv_sim"][0], o["v_opt"][0], o["w_opt"][0], p.robot_radius, pol)
        rows.append(row)
        i += 1
    return B._result(rows, st, u1, u2, i, pol)


def engine(K, H, seed, plan=None, k_offset=0, **kw):
    """An engine on the C3 scene with `plan` set (None: never touched)."""
    Z, hw, cm = hp.c3_scene()
    eng = hp.engine_for(K, H, Z, hw, cm, hp.oracle_state(wl=0.3, wr=0.5, goal=FAR), seed=seed, k_offset=k_offset, **kw)
    if plan is not None:
        eng.set_sampling(**plan)
    return eng
