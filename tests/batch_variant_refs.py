"""References for per-episode parameter variants and on-device scoring of batched episodes
(tests/test_gpu_batch_variants.py, tests/test_gpu_batch_score.py).

An episode that holds a variant must be, step for step, the closed loop of a context created with
the batch context's params overridden by the variant (mppi_amd.batch.variant_params):

  reference A  batch_refs.oracle_loop with oracle Params built from the overridden parameter set
  reference B  a fresh Engine(make_params(K, H, seed=..., **overridden)) stepped from the host with
               batch_refs.rule

The variants below are those of the issue.  On the CPU oracle (seed 7, 8 steps, run() policy, start
(-60, -5), goal (65, 10), heading (1, 0, 0)) each changes at least 6 of the 8 log rows against the
default 3D run, so a variant that is silently ignored cannot pass; the collision variant only acts
from COLLISION_START, which has an obstacle in reach.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import batch_refs as B
from oracle import mppi_ref as R

F32 = np.float32
K, H, SEED, CAP = 256, 20, 7, 8
FAR = (65.0, 10.0)
COLLISION_START = (-38.7, 39.7)
WEIGHTS = ("w_path", "w_slope", "w_speed", "w_obstacle")

# name -> (projection, variant fields that differ from the defaults, start)
VARIANTS = {
    "proj2d": ("2d", {}, B.START),
    "weights": ("3d", dict(w_slope=0.0, w_obstacle=100.0, w_speed=5.0), B.START),
    "temperature3": ("3d", dict(temperature=3.0), B.START),
    "temperature3000": ("3d", dict(temperature=3000.0), B.START),     # the dense leaf arm
    "filters": ("3d", dict(filter_k=3.0, filter_a=0.9, opt_filter_k=2.5, opt_filter_a=0.85), B.START),
    "isaac_sigma": ("3d", dict(sigma_base=0.25, sigma_div=3.0), B.START),
    "collision": ("3d", dict(collision_threshold=0.5, collision_penalty=1000.0), COLLISION_START),
}


def variant(name):
    """The full variant dict (mppi_batch_variant fields + proj) of VARIANTS[name]."""
    from mppi_amd.batch import variant_dict
    proj, fields, _ = VARIANTS[name]
    return variant_dict(proj, **fields)


def overridden(var, pol=B.RUN, proj="3d"):
    """(params dict, policy dict, proj) an episode with variant dict `var` (None: no variant) runs with."""
    from mppi_amd.batch import variant_params
    return variant_params({}, var, pol, proj)


def ref_a(start, goal, seed, n_steps, var, pol=B.RUN, proj="3d", k=K, h=H):
    """Reference A: the oracle loop with the overridden parameter set."""
    from helpers import c3_scene, oracle_scene
    params, pol, proj = overridden(var, pol, proj)
    p = R.Params(**{k_: float(v) for k_, v in params.items()})
    return B.oracle_loop(k, h, oracle_scene(*c3_scene()), B.start_state(start, goal), seed, n_steps, proj, pol, params=p)


def ref_b(start, goal, seed, n_steps, var, pol=B.RUN, proj="3d", k=K, h=H):
    """Reference B: a fresh engine created with the overridden params, stepped from the host."""
    from helpers import c3_scene
    from mppi_amd import _lib
    params, pol, proj = overridden(var, pol, proj)
    Z, hw, cm = c3_scene()
    st = B.start_state(start, goal)
    eng = _lib.Engine(_lib.make_params(k, h, seed=seed, **{k_: float(v) for k_, v in params.items()}), 0)
    try:
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        r = float(eng.params.robot_radius)
        rows = []
        i = 0
        while i < n_steps and B.active(st, pol):
            eng.set_state(_lib.make_state(st["x"], st["y"], st["heading"], st["wl"], st["wr"], st["gx"], st["gy"],
                                          st["s1"], st["s2"]))
            o = eng.step(proj, i)
            st, row = B.rule(st, o["traj_sim"][0], o["heading_sim"][0], o["lin_vel"][0], o["ang_vel"][0], r, pol)
            rows.append(row)
            i += 1
        u1, u2 = eng.get_nominal()
    finally:
        eng.close()
    return B._result(rows, st, u1, u2, i, pol)


@functools.lru_cache(maxsize=None)
def ref_a_named(name):
    """Reference A of the main case's episode `name` (a VARIANTS key, "default" or "default_collision"),
    computed once per session."""
    if name == "default":
        return ref_a(B.START, FAR, SEED, CAP, None)
    if name == "default_collision":
        return ref_a(COLLISION_START, FAR, SEED, CAP, None)
    return ref_a(VARIANTS[name][2], FAR, SEED, CAP, variant(name))


def mppi_state(st):
    """The ctypes MppiState of a batch_refs state dict (the heading used as given)."""
    from mppi_amd import _lib
    s = _lib.MppiState()
    s.x, s.y = float(st["x"]), float(st["y"])
    for i in range(3):
        s.heading[i] = float(np.float32(st["heading"][i]))
    s.left_wheel_speed, s.right_wheel_speed = float(st["wl"]), float(st["wr"])
    s.goal_x, s.goal_y = float(st["gx"]), float(st["gy"])
    s.std_dev_u1, s.std_dev_u2 = float(st["s1"]), float(st["s2"])
    return s


def collect(batch, e):
    """What a batch reports of episode e, in the layout of batch_refs._result."""
    info = batch.episode(e)
    s = info["state"]
    final = np.array([s.x, s.y, s.heading[0], s.heading[1], s.heading[2], s.left_wheel_speed, s.right_wheel_speed,
                      s.goal_x, s.goal_y, s.std_dev_u1, s.std_dev_u2], np.float32)
    return dict(rows=batch.log(e), final=final, u1=info["u1"], u2=info["u2"], steps=info["steps_last_run"],
                total=info["steps_total"], reached=info["reached"])


def same(got, ref, tag):
    assert got["steps"] == ref["steps"], (tag, got["steps"], ref["steps"])
    assert got["reached"] == ref["reached"], tag
    for k_, what in (("rows", "log rows"), ("final", "final state"), ("u1", "nominal u1"), ("u2", "nominal u2")):
        g, w = np.asarray(got[k_], F32), np.asarray(ref[k_], F32)
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{what} {tag}"


def differ(a, b):
    """Rows of two logs of equal length that are not bitwise equal."""
    assert a["rows"].shape == b["rows"].shape
    return int((a["rows"].view(np.uint32) != b["rows"].view(np.uint32)).any(axis=1).sum())


def make_engine(k=K, h=H, **params):
    from helpers import c3_scene
    from mppi_amd import _lib
    Z, hw, cm = c3_scene()
    eng = _lib.Engine(_lib.make_params(k, h, **params), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    return eng


# ---- scoring ----

def origin_state(x, y, gx, gy):
    from mppi_amd import _lib
    return _lib.make_state(x, y, (1.0, 0.0, 0.0), 0.0, 0.0, gx, gy)


def score_one(engine, rows, origin):
    """mppi_score_paths on one logged path (traj = columns 0-2, lin_vel = column 6, no wheels) from
    `origin` (MppiState); a path without rows scores zero."""
    if len(rows) == 0:
        return dict(cost=F32(0), terms=np.zeros(4, F32), collisions=np.int32(0))
    r = engine.score_paths(np.ascontiguousarray(rows[None, :, 0:3]), np.ascontiguousarray(rows[None, :, 6]),
                           state=origin)
    return dict(cost=r["cost"][0], terms=r["terms"][0], collisions=r["collisions"][0])


def check_scores(got, engine, logs, origins, tag):
    """Batch.score()'s dict against score_one per episode, bitwise."""
    E = len(logs)
    assert got["cost"].shape == (E,) and got["terms"].shape == (E, 4)
    assert got["collisions"].shape == (E,) and got["rows"].shape == (E,)
    for e in range(E):
        want = score_one(engine, logs[e], origins[e])
        assert got["rows"][e] == len(logs[e]), (tag, e)
        assert F32(got["cost"][e]).view(np.uint32) == F32(want["cost"]).view(np.uint32), \
            (tag, e, got["cost"][e], want["cost"])
        assert np.array_equal(got["terms"][e].view(np.uint32), np.asarray(want["terms"], F32).view(np.uint32)), \
            (tag, e, got["terms"][e], want["terms"])
        assert got["collisions"][e] == want["collisions"], (tag, e)


def oracle_terms(rows, origin_xy, goal, horizon):
    """(terms [4], collisions) of one logged path from oracle.mppi_ref.critics in body-slope mode
    (lw = rw = traj), each critic from the same function with its weight 1 and the others 0."""
    from helpers import c3_scene
    Z, hw, cm = c3_scene()
    sc = R.Scene(Z, hw, cm)
    traj = np.ascontiguousarray(rows[None, :, 0:3], dtype=F32)
    v = np.ascontiguousarray(rows[None, :, 6], dtype=F32)
    p = R.Params(K=1, H=len(rows), horizon=horizon)
    st = R.State(x=float(origin_xy[0]), y=float(origin_xy[1]), goal_x=float(goal[0]), goal_y=float(goal[1]))
    terms = np.stack([R.critics(dataclasses.replace(p, **{w: (1.0 if w == one else 0.0) for w in WEIGHTS}),
                                sc, st, traj, traj, traj, v) for one in WEIGHTS], -1)[0].astype(F32)
    col = int((R.costmap_at(sc, traj[:, :, 0], traj[:, :, 1]) > p.f("collision_threshold")).sum())
    return terms, col
