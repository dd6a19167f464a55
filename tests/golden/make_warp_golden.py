"""Generate tests/golden/ref_warp_steps.npz: whole MPPI steps of the REFERENCE'S OWN Warp code.

Run by hand in the build container only (it needs the reference tree, see make_golden.py):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_warp_golden.py

The reference's kernels (thesis_master/warp_implementation/critics_warp.py, projection_warp.py,
sampling_warp.py) and its host class (MPPI_isaac.py) are imported from the read-only reference tree
with the project's stand-in (oracle/warp_standin.py) in ``sys.modules["warp"]`` and
an empty module in ``sys.modules["cv2"]``.  Nothing of the reference is stored but numbers.

What runs is the reference's: ``Surface`` (``which_map="manual"``: its own ``create_surface``; a costmap
mode that is neither "manual" nor "imported", so no cv2, and ``.costmap`` assigned afterwards),
``Robot`` and ``MPPI_Controller`` from a YAML config written to a temporary file, and then its own
``run(proj)``, i.e. ``warp_setup``, and per loop ``reset("controller")``, ``MPPI_step(proj)`` and the
feedback of the state (the robot moves to row 0 of ``traj_sim``; heading, wheel speeds and sigmas
follow).  ``run`` is entered with its loop counter ``steps`` short of its cap, so it makes exactly
``steps`` loops.  The generator only listens: ``MPPI_step`` is wrapped to copy the arrays before and
after the reference's call, and the controller's ``rng`` to note the seed it draws.

Two things are the generator's own, both flagged in the fixture's ``meta``:

* ``settled_minimum``.  ``_compute_weights`` (critics_warp.py:338-347) races by design: a thread
  reads ``min_cost[0]`` while other threads still lower it.  Both of its writes are idempotent, so
  the generator launches that kernel a SECOND time with the same arguments; the weights are then
  taken against the true minimum.  That is what a GPU gives once the minimum has settled, and it is
  the project's definition.  In ascending thread order the first launch alone
  would give every thread that lowers the minimum the weight 1.
* ``nominal``.  Some cases start from a previous optimum that is not zero; it is written into
  ``optimal_u1_wp`` / ``optimal_u2_wp`` with the arrays' ``assign`` after ``warp_setup``.

Every case asserts, on the reference's own arrays, that it exercises what it is named for, and that
every waypoint and wheel stays at least one cell inside the DEM (the stand-in's arrays raise on an
index outside; a column that runs over into the next row would not, so the margin is asserted).
Outside the map the reference reads out of bounds and the project clamps (D3): no fixture goes there.

Output, ``ref_warp_steps.npz`` (K = 64, one case K = 65, H <= 24; one 160^2 DEM from
``create_surface`` and one 20^2 costmap, shared):

  Z, costmap, half_width
  <case>/meta         JSON: config, proj, math table, seed, state (x, y, heading as used, wheel
                      speeds, goal, sigmas), flags
  <case>/randn_table  the float32 table ``randn`` read, /randn_states the states asked for, in order
  <case>/u_nom1,2     optimal_u* before the step
  <case>/u1 u2 v w [K, H]; traj hv lw rw [K, H, 3]; costs weights [K]; weights_sum [1];
  <case>/terms [K, 4] the four launched critics called as plain functions (unweighted)
  <case>/optimal_u1 optimal_u2 v_opt w_opt [H]; traj_sim hv_sim lw_sim rw_sim [H, 3]
  <case>/alt_slope alt_orientation [K]   (far3d, within_horizon) ``_avoid_slope`` and
                      ``_path_orientation_critic`` called as plain functions: the reference launches neither
  libm/<case>/...     final results of two cases under the "libm" math table, and in meta the largest
                      relative difference of the costs from the "project" run (measured, not asserted)
"""
from __future__ import annotations

import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_golden import REF_DEBUG  # noqa: E402  (one place names the reference tree)
from oracle import warp_standin as W  # noqa: E402

F32 = np.float32
REF_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(REF_DEBUG)))
OUT = os.path.join(HERE, "ref_warp_steps.npz")

GRID, HALF_WIDTH, CM_SIZE = 160, 20.0, 20           # Surface: costmap_size = int(grid_size / 8)
STEP_ARRAYS = ("u1", "u2", "v", "w", "traj", "hv", "lw", "rw", "costs", "weights", "weights_sum", "terms",
               "optimal_u1", "optimal_u2", "v_opt", "w_opt", "traj_sim", "hv_sim", "lw_sim", "rw_sim")
FINAL_ARRAYS = ("costs", "optimal_u1", "optimal_u2", "v_opt", "w_opt")

# the reference's config.yaml values (the project's defaults: oracle.mppi_ref.Params), at K = 64
CONFIG = dict(robot_radius=1.2, H=12, dt=0.045, K=64, initial_linear_velocity=0.0, min_linear_velocity=0.0,
              max_linear_velocity=2.0, initial_angular_velocity=0.0, min_angular_velocity=-1.0,
              max_angular_velocity=1.0, std_dev_u1=0.25, std_dev_u2=0.25, min_u1=-1.0, max_u1=1.0, min_u2=-1.0,
              max_u2=1.0, temperature=0.3)


def reference_present():
    return os.path.isdir(os.path.join(REF_ROOT, "thesis_master", "warp_implementation"))


# ------------------------------------------------------------------ the scene
def bumps():
    from mppi_amd import scene
    return [((cx * 0.25, cy * 0.25), h, w * 0.25) for (cx, cy), h, w in scene.BUMPS_9]


def costmap(size=CM_SIZE, seed=1):
    """uniform(0, 1) with a tenth of the cells at 0.995 (tests/test_gpu_param_space._costmap)."""
    rng = np.random.default_rng(seed)
    cm = rng.uniform(0.0, 1.0, (size, size)).astype(F32)
    cm[rng.uniform(size=cm.shape) < 0.1] = 0.995
    return cm


# ------------------------------------------------------------------ the reference under the stand-in
def load_reference(math_table):
    """(stand-in, MPPI_isaac, critics_warp) imported afresh, so that their ``wp`` is this stand-in."""
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True                  # the reference tree is read-only
    wp = W.create(math_table)

    def purge():
        for m in [m for m in sys.modules if m == "thesis_master" or m.startswith("thesis_master.")]:
            del sys.modules[m]

    saved = {k: sys.modules.get(k) for k in ("warp", "cv2")}
    purge()
    sys.modules["warp"] = wp
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, REF_ROOT)
    try:
        M = importlib.import_module("thesis_master.warp_implementation.MPPI_isaac")
        C = importlib.import_module("thesis_master.warp_implementation.critics_warp")
    finally:
        sys.path.remove(REF_ROOT)
        purge()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    real_launch = wp.launch
    wp.relaunched = []

    def launch(kernel=None, dim=None, inputs=(), **kw):
        real_launch(kernel=kernel, dim=dim, inputs=inputs, **kw)
        if kernel.__name__ == "_compute_weights":   # settled_minimum (see the module's text)
            first = inputs[2].numpy()
            real_launch(kernel=kernel, dim=dim, inputs=inputs, **kw)
            wp.relaunched.append(int((first != inputs[2].numpy()).sum()))

    wp.launch = launch
    return wp, M, C


class _NotedRng:
    def __init__(self, rng):
        self.rng = rng
        self.drawn = []

    def integers(self, *a, **kw):
        v = self.rng.integers(*a, **kw)
        self.drawn.append(int(v))
        return v


def _yaml(cfg):
    return dict(frame_work=dict(robot_radius=cfg["robot_radius"]),
                controller=dict(number_of_iterations=cfg["H"], dt=cfg["dt"], number_of_trajectories=cfg["K"]),
                velocities={k: cfg[k] for k in ("initial_linear_velocity", "min_linear_velocity", "max_linear_velocity",
                                                "initial_angular_velocity", "min_angular_velocity",
                                                "max_angular_velocity")},
                inputs={k: cfg[k] for k in ("std_dev_u1", "min_u1", "max_u1", "std_dev_u2", "min_u2", "max_u2")},
                cost_evaluation=dict(temperature=cfg["temperature"]))


def run_reference(ref, spec, steps=1):
    """The reference's ``run`` for ``steps`` loops of the case ``spec``; one record per step."""
    import yaml
    wp, M, C = ref
    cfg = {**CONFIG, **spec.get("config", {})}
    K, H, proj = cfg["K"], cfg["H"], spec.get("proj", "3d")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "config.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(_yaml(cfg), f)
        surface = M.Surface("manual", None, "assigned", None, GRID, HALF_WIDTH, (0.0, 0.0), bumps(),
                            cfg["robot_radius"])
        surface.costmap = costmap()
        robot = M.Robot(spec["start"][0], spec["start"][1], list(spec["heading"]), path)
        robot.left_wheel_speed, robot.right_wheel_speed = spec.get("wheels", (0.0, 0.0))
        ctrl = M.MPPI_Controller(surface, robot, path, spec["goal"][0], spec["goal"][1], 0.0)
    ctrl.rng = _NotedRng(ctrl.rng)
    table = np.random.default_rng(spec["table_seed"]).standard_normal(1000 + K * H + 4 * H + 1).astype(F32)
    nominal = None
    if spec.get("nominal_seed") is not None:
        r = np.random.default_rng(spec["nominal_seed"])
        nominal = (r.uniform(-0.6, 0.6, H).astype(F32), r.uniform(-0.6, 0.6, H).astype(F32))
    records = []
    step_fn = ctrl.MPPI_step

    def listening_step(proj):
        if nominal is not None and not records:
            ctrl.optimal_u1_wp.assign(nominal[0])
            ctrl.optimal_u2_wp.assign(nominal[1])
        hv0 = ctrl.previous_heading_vector
        state = dict(x=float(F32(robot.x[-1])), y=float(F32(robot.y[-1])), heading=[float(c) for c in hv0],
                     left_wheel_speed=float(F32(robot.left_wheel_speed)),
                     right_wheel_speed=float(F32(robot.right_wheel_speed)), goal_x=float(F32(ctrl.goal_x)),
                     goal_y=float(F32(ctrl.goal_y)), std_dev_u1=float(F32(ctrl.std_dev_u1)),
                     std_dev_u2=float(F32(ctrl.std_dev_u2)))
        rec = dict(u_nom1=ctrl.optimal_u1_wp.numpy(), u_nom2=ctrl.optimal_u2_wp.numpy(), randn_table=table)
        wp.randn_table = table
        wp.randn_states = []
        del wp.relaunched[:]
        drawn = len(ctrl.rng.drawn)
        step_fn(proj=proj)
        assert len(wp.relaunched) == 1 and len(ctrl.rng.drawn) == drawn + 1
        rec["randn_states"] = np.asarray(wp.randn_states, np.int32)
        shape2, shape3 = (K, H), (K, H, 3)
        rec.update(u1=ctrl.u1.numpy().reshape(shape2), u2=ctrl.u2.numpy().reshape(shape2),
                   v=ctrl.linear_velocities.numpy().reshape(shape2), w=ctrl.angular_velocities.numpy().reshape(shape2),
                   traj=ctrl.trajectories.numpy().reshape(shape3), hv=ctrl.heading_vectors.numpy().reshape(shape3),
                   lw=ctrl.left_wheel_pos.numpy().reshape(shape3), rw=ctrl.right_wheel_pos.numpy().reshape(shape3),
                   costs=ctrl.costs_wp.numpy(), weights=ctrl.weights_wp.numpy(), weights_sum=ctrl.weights_sum.numpy(),
                   optimal_u1=ctrl.optimal_u1_wp.numpy(), optimal_u2=ctrl.optimal_u2_wp.numpy(),
                   v_opt=ctrl.optimal_lin_vel_wp.numpy(), w_opt=ctrl.optimal_ang_vel_wp.numpy(),
                   traj_sim=ctrl.trajectories_sim.numpy(), hv_sim=ctrl.heading_vectors_sim.numpy(),
                   lw_sim=ctrl.left_wheel_pos_sim.numpy(), rw_sim=ctrl.right_wheel_pos_sim.numpy())
        # the critics as plain functions, with the evaluation kernel's own arguments (critics_warp.py:325-329)
        x, y, it = robot.x[-1], robot.y[-1], wp.float(H)
        terms = np.zeros((K, 4), F32)
        alt = np.zeros((K, 2), F32)
        for t in range(K):
            s = wp.float(t) * it
            terms[t, 0] = C._path_follow_critic(x, y, ctrl.goal, ctrl.trajectories, s, it, ctrl.horizon)
            terms[t, 1] = C._avoid_slope_wheels(ctrl.left_wheel_pos, ctrl.right_wheel_pos, s, it)
            terms[t, 2] = C._maximise_speed(x, y, ctrl.goal, ctrl.linear_velocities, ctrl.v_max_linear, s, it,
                                            ctrl.horizon)
            terms[t, 3] = C._avoid_obstacle(ctrl.trajectories, s, it, surface.half_width, surface.costmap_resolution,
                                            surface.costmap_size, ctrl.costmap_wp)
            if spec.get("alt"):
                alt[t, 0] = C._avoid_slope(ctrl.trajectories, s, it)
                alt[t, 1] = C._path_orientation_critic(x, y, ctrl.goal, ctrl.trajectories, s, it)
        rec["terms"] = terms
        if spec.get("alt"):
            rec["alt_slope"], rec["alt_orientation"] = alt[:, 0].copy(), alt[:, 1].copy()
        rec["meta"] = dict(config=cfg, proj=proj, math=wp.math_table, seed=ctrl.rng.drawn[-1], state=state,
                           horizon=float(ctrl.horizon), settled_minimum=True,
                           weights_changed_by_second_launch=wp.relaunched[0], nominal=nominal is not None,
                           step=len(records))
        records.append(rec)

    ctrl.MPPI_step = listening_step
    ctrl.loop = 3500 - steps                         # run()'s cap: exactly ``steps`` loops
    with contextlib.redirect_stdout(io.StringIO()):
        ctrl.run(proj)
    assert len(records) == steps, (len(records), steps)
    for rec in records:
        _assert_inside(rec)
    return records, surface


def _assert_inside(rec):
    """Every waypoint and wheel at least one DEM cell inside the map (so inside the costmap too)."""
    res = 2 * HALF_WIDTH / GRID
    pts = [rec["traj"], rec["traj_sim"], rec["lw_sim"], rec["rw_sim"]]
    if rec["meta"]["proj"] == "3d":
        pts += [rec["lw"], rec["rw"]]
    for a in pts:
        xy = a[..., :2]
        assert np.isfinite(a).all() and np.abs(xy).max() < HALF_WIDTH - 2 * res, "the case leaves the map"
    for k in STEP_ARRAYS:
        assert np.isfinite(rec[k]).all(), k


# ------------------------------------------------------------------ the cases
def _collision_start():
    """A start 0.2 m to 1.2 m west of a cell above the threshold, heading east into it, chosen so that
    about half of the oracle's rollouts reach the cell.  (The oracle only picks the spot; the case's
    assertion is on the reference's arrays.)"""
    cm = costmap()
    res_c = 2 * HALF_WIDTH / CM_SIZE
    rows, cols = np.nonzero(cm > 0.99)
    for j, i in zip(rows, cols):
        if 5 <= i < CM_SIZE - 3 and 3 <= j < CM_SIZE - 3 and cm[j, i - 1] <= 0.99:
            break
    else:
        raise AssertionError("no such cell")
    edge = -HALF_WIDTH + i * res_c
    y = HALF_WIDTH - (j + 0.5) * res_c
    return edge, y


CASES = {
    "far3d": dict(start=(5.3, 6.4), heading=(-1.0, -0.5, 0.0), wheels=(0.4, 0.6), goal=(-15.0, -8.0), table_seed=101,
                  config=dict(H=16), alt=True),
    "far2d": dict(proj="2d", start=(5.3, 6.4), heading=(1.0, 0.4, 0.0), wheels=(0.5, 0.3), goal=(15.0, 9.0),
                  table_seed=102),
    "chain3": dict(start=(-12.0, 3.0), heading=(1.0, 0.2, 0.0), wheels=(0.3, 0.3), goal=(15.0, 5.0), table_seed=103,
                   steps=3),
    "within_horizon": dict(start=(8.0, -9.0), heading=(-0.2, 1.0, 0.0), wheels=(0.8, 0.7), goal=(10.0, -9.6),
                           table_seed=104, config=dict(H=24), alt=True),
    "near_goal": dict(start=(-6.0, 7.5), heading=(0.0, -1.0, 0.0), wheels=(0.2, 0.4), goal=(-5.0, 6.4), table_seed=105),
    "collisions": dict(heading=(1.0, 0.0, 0.0), wheels=(1.6, 1.6), goal=(15.0, 5.0), table_seed=106,
                       config=dict(std_dev_u1=1.0, std_dev_u2=1.0)),
    "negative_quadrant": dict(start=(-7.3, -9.6), heading=(0.6, -0.7, 0.3), wheels=(0.9, 1.0), goal=(-15.0, -14.0),
                              table_seed=107, nominal_seed=7),
    "reverse": dict(start=(3.0, -4.0), heading=(-1.0, 1.0, 0.0), goal=(12.0, 9.0), table_seed=108,
                    config=dict(min_linear_velocity=-1.0, std_dev_u1=0.5, std_dev_u2=0.5)),
    "large_angle": dict(start=(2.0, 3.0), heading=(0.0, 1.0, 0.0), wheels=(-0.47, 0.47), goal=(-14.0, 10.0),
                        table_seed=109, config=dict(dt=0.25, robot_radius=0.3, min_angular_velocity=-6.0,
                                                    max_angular_velocity=6.0, std_dev_u1=1.0, std_dev_u2=1.0)),
    "limits": dict(start=(-3.0, 11.0), heading=(1.0, 1.0, 0.0), wheels=(0.6, 0.2), goal=(14.0, -3.0), table_seed=110,
                   nominal_seed=10, config=dict(min_u1=-0.3, max_u1=0.9, min_u2=-0.7, max_u2=0.2, std_dev_u1=0.6,
                                                std_dev_u2=0.6)),
    "odd": dict(start=(11.0, 2.0), heading=(-1.0, -0.1, 0.0), wheels=(0.5, 0.5), goal=(-9.0, -12.0), table_seed=111,
                nominal_seed=11, config=dict(K=65, H=9)),
}
LIBM_CASES = ("collisions", "large_angle")   # exp in the weights of both; large_angle: sin / cos up to 1.5 rad


def _frac(mask):
    return float(np.mean(mask))


def check_case(name, records):
    """The case exercises what it is named for: asserted on the reference's own arrays."""
    r = records[0]
    m = r["meta"]
    st, cfg = m["state"], m["config"]
    dist = float(np.hypot(st["goal_x"] - st["x"], st["goal_y"] - st["y"]))
    collided = r["terms"][:, 3] >= 100000.0
    if name in ("far3d", "far2d"):
        assert cfg == {**CONFIG, "H": cfg["H"]} and dist > m["horizon"] and m["proj"] == name[-2:]
        if name == "far2d":
            assert not r["lw"].any() and not r["rw"].any()
    if name == "chain3":
        assert len(records) == 3
        for a, b in zip(records, records[1:]):       # the feedback of run(): :769-784
            sa, sb = a["meta"]["state"], b["meta"]["state"]
            assert (sb["x"], sb["y"]) == (float(a["traj_sim"][0, 0]), float(a["traj_sim"][0, 1]))
            assert (sb["x"], sb["y"]) != (sa["x"], sa["y"]) and sb["heading"] != sa["heading"]
            assert sb["left_wheel_speed"] != sa["left_wheel_speed"]
            assert np.array_equal(b["u_nom1"], a["optimal_u1"]) and np.array_equal(b["u_nom2"], a["optimal_u2"])
            assert a["optimal_u1"].any() and a["optimal_u2"].any()
            assert b["meta"]["seed"] != a["meta"]["seed"]
    if name == "within_horizon":
        assert 2.0 <= dist <= m["horizon"], (dist, m["horizon"])
        assert (r["terms"][:, 2] != 0).all()          # the speed critic is still on
    if name == "near_goal":
        assert dist < 2.0 and not r["terms"][:, 2].any()
    else:
        assert r["terms"][:, 2].any()
    if name == "collisions":
        assert 0.05 <= _frac(collided) and 0.05 <= _frac(~collided), _frac(collided)
    if name == "negative_quadrant":
        assert (r["traj"][..., :2] < 0).all() and (r["lw"][..., :2] < 0).all() and (r["rw"][..., :2] < 0).all()
        assert st["x"] < 0 and st["y"] < 0 and abs(st["heading"][2]) > 0.1
    if name == "reverse":
        assert cfg["min_linear_velocity"] < 0
        assert _frac(r["v"] > 0) >= 0.25 and _frac(r["v"] < 0) >= 0.25, (_frac(r["v"] > 0), _frac(r["v"] < 0))
    if name == "large_angle":
        assert min(-cfg["min_angular_velocity"], cfg["max_angular_velocity"]) * cfg["dt"] > np.pi / 4
        big = np.abs(r["w"] * F32(cfg["dt"])) > np.pi / 4
        assert 0.1 <= _frac(big) <= 0.9, _frac(big)    # both arms of the range reduction, j = 0 and j > 0
    if name == "limits":
        assert -cfg["min_u1"] != cfg["max_u1"] and -cfg["min_u2"] != cfg["max_u2"]
        for u, lo, hi in ((r["u1"], cfg["min_u1"], cfg["max_u1"]), (r["u2"], cfg["min_u2"], cfg["max_u2"])):
            assert _frac(u == F32(lo)) >= 0.01 and _frac(u == F32(hi)) >= 0.01
            assert _frac((u > F32(lo)) & (u < F32(hi))) >= 0.25
    if name == "odd":
        assert (cfg["K"], cfg["H"]) == (65, 9)
    if m["nominal"]:
        assert r["u_nom1"].any() and r["u_nom2"].any()
    assert cfg["H"] <= 24 and cfg["K"] in (64, 65)
    assert len(np.unique(r["costs"])) > cfg["K"] // 2, "degenerate costs"


def make_case(name, math_table="project", ref=None):
    """The records of one case (a list, one per step), checked."""
    spec = dict(CASES[name])
    if name == "collisions":
        spec["start"] = _collision_search(spec)
    ref = ref or load_reference(math_table)
    records, _ = run_reference(ref, spec, spec.get("steps", 1))
    check_case(name, records)
    return records


def _collision_search(spec):
    """Distance from the hot cell's edge at which about half of the oracle's rollouts reach it."""
    from oracle import mppi_ref as R
    edge, y = _collision_start()
    cfg = {**CONFIG, **spec["config"]}
    K, H = cfg["K"], cfg["H"]
    p = R.Params(K=K, H=H)
    table = np.random.default_rng(spec["table_seed"]).standard_normal((K, H)).astype(F32)
    best = None
    for d in np.arange(0.2, 1.4, 0.05):
        st = R.State(x=edge - d, y=y, heading=np.asarray(spec["heading"], float), left_wheel_speed=spec["wheels"][0],
                     right_wheel_speed=spec["wheels"][1], std_dev_u1=cfg["std_dev_u1"], std_dev_u2=cfg["std_dev_u2"])
        u1, u2 = R.sample_controls(p, st, np.zeros(H, F32), np.zeros(H, F32), table, table[::-1])
        v, _ = R.wheel_filter(p, st, u1, u2, p.filter_k, p.filter_a)
        reach = st.x + np.cumsum(v * F32(cfg["dt"]), axis=1)[:, -1]
        f = float(np.mean(reach >= edge))
        if best is None or abs(f - 0.5) < abs(best[0] - 0.5):
            best = (f, float(F32(edge - d)))
    return (best[1], float(F32(y)))


def _keys(prefix, rec, arrays):
    out = {f"{prefix}/meta": np.array(json.dumps(rec["meta"], sort_keys=True))}
    for k in arrays:
        if k in rec:
            out[f"{prefix}/{k}"] = rec[k]
    return out


def case_entries(name, records):
    """The .npz entries of a case: ``name/...``, or ``name.<step>/...`` for a chain."""
    every = ("randn_table", "randn_states", "u_nom1", "u_nom2", "alt_slope", "alt_orientation") + STEP_ARRAYS
    out = {}
    for i, rec in enumerate(records):
        out.update(_keys(name if len(records) == 1 else f"{name}.{i}", rec, every))
    return out


def main():
    assert reference_present(), "the reference tree is needed to generate this fixture"
    ref = load_reference("project")
    data = {}
    project = {}
    surface = None
    for name in CASES:
        records = make_case(name, ref=ref)
        project[name] = records
        assert all(r["meta"]["math"] == "project" for r in records)
        data.update(case_entries(name, records))
        r = records[0]
        print(f"{name}: K={r['meta']['config']['K']} H={r['meta']['config']['H']} steps={len(records)} "
              f"seed={r['meta']['seed']} collided={int((r['terms'][:, 3] >= 1e5).sum())} "
              f"weights changed by the second launch={r['meta']['weights_changed_by_second_launch']}")
    libm = load_reference("libm")
    for name in LIBM_CASES:
        rec = make_case(name, "libm", ref=libm)[0]
        base = project[name][0]
        for k in ("u1", "u2", "v", "w"):             # no transcendental before the rollout
            assert np.array_equal(rec[k], base[k]), k
        c0, c1 = base["costs"].astype(np.float64), rec["costs"].astype(np.float64)
        rec["meta"]["cost_rel_diff_from_project_max"] = float(np.max(np.abs(c1 - c0) / np.abs(c0)))
        rec["meta"]["costs_equal_to_project"] = int((c0 == c1).sum())
        data.update(_keys(f"libm/{name}", rec, FINAL_ARRAYS))
        print(f"libm/{name}: max relative cost difference from the project table "
              f"{rec['meta']['cost_rel_diff_from_project_max']:.3e}, {rec['meta']['costs_equal_to_project']} of "
              f"{c0.size} costs equal")
    _, M, _ = ref
    with contextlib.redirect_stdout(io.StringIO()):
        surface = M.Surface("manual", None, "assigned", None, GRID, HALF_WIDTH, (0.0, 0.0), bumps(), 1.2)
    data["Z"] = surface.Z.astype(F32)
    data["costmap"] = costmap()
    data["half_width"] = np.float64(HALF_WIDTH)
    np.savez_compressed(OUT, **data)
    print("ref_warp_steps.npz:", os.path.getsize(OUT), "bytes,", len(data), "entries")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
