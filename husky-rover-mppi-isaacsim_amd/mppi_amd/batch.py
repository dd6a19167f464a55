"""The closed loop's advance rule (MPPI_Controller.run, MPPI_isaac.py:769-784), explicit.

This is the host's half of the contract of the batched episodes (include/mppi.h, mppi_batch_*;
DESIGN.md §3.7): the finish-and-advance kernel applies the same arithmetic on the GPU after every
step.  Plain numpy float32 / float64, usable without a GPU or the library.

A state is a dict with the fields of mppi_state: x, y, heading (3 values), left_wheel_speed,
right_wheel_speed, goal_x, goal_y, std_dev_u1, std_dev_u2.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32

RUN_POLICY = dict(sigma_base=0.4, sigma_div=1.0, goal_tol=0.5)      # MPPI_isaac.py:763-784
ISAAC_POLICY = dict(sigma_base=0.25, sigma_div=3.0, goal_tol=0.5)   # visual_terrain_stack_full_terrain.py:510-511

STATE_FIELDS = ("x", "y", "heading", "left_wheel_speed", "right_wheel_speed", "goal_x", "goal_y",
                "std_dev_u1", "std_dev_u2")


# mppi_batch_variant (include/mppi.h): the mppi_params fields a variant overrides, then the loop
# policy's sigma schedule and the projection
VARIANT_PARAM_FIELDS = ("w_path", "w_slope", "w_speed", "w_obstacle", "collision_threshold", "collision_penalty",
                        "temperature", "filter_k", "filter_a", "opt_filter_k", "opt_filter_a")
VARIANT_POLICY_FIELDS = ("sigma_base", "sigma_div")


def variant_params(params, variant, policy=None, proj="3d"):
    """What an episode that holds `variant` runs with: (params dict, policy dict, proj).

    params: the batch context's parameters by mppi_params field name (any mapping; fields not
    given keep the library's defaults when passed on to make_params); variant: dict of
    mppi_batch_variant fields, or None for an episode without a variant; policy, proj: those of
    mppi_batch_run.  Exactly VARIANT_PARAM_FIELDS are overridden in params, sigma_base / sigma_div in
    the policy (goal_tol and check_every stay the run's), and proj by the variant's ("2d" / "3d" or
    2 / 3).  A variant must give every field, as the C struct does; Batch.variant_default or
    _lib.make_variant fill them.
    """
    out = dict(params)
    pol = dict(policy or RUN_POLICY)
    if variant is None:
        return out, pol, proj
    v = dict(variant)
    known = set(VARIANT_PARAM_FIELDS) | set(VARIANT_POLICY_FIELDS) | {"proj"}
    if set(v) != known:
        raise ValueError(f"a variant gives exactly {sorted(known)}; got {sorted(v)}")
    for k in VARIANT_PARAM_FIELDS:
        out[k] = F32(v[k])
    for k in VARIANT_POLICY_FIELDS:
        pol[k] = F32(v[k])
    if not pol["sigma_div"] != 0:
        raise ValueError("sigma_div must be non-zero")
    if not out["temperature"] > 0:
        raise ValueError("temperature must be > 0")
    pj = {2: "2d", 3: "3d", "2d": "2d", "3d": "3d"}.get(v["proj"])
    if pj is None:
        raise ValueError("proj must be 2 or 3")
    return out, pol, pj


CRITIC_FIELDS = ("slope", "w_orientation")     # mppi_critics (include/mppi.h), by Engine.set_critics' names


def split_variant(variant):
    """A variant dict that may carry the critic keys -> (the mppi_batch_variant dict, the critic set).

    "slope" ("wheels" | "body") and "w_orientation" are not fields of mppi_batch_variant: they fill
    the batch's second table (mppi_batch_set_variant_critics).  The critic set is
    dict(slope=, w_orientation=) with "wheels" / 0.0 for a key not given, or None when the dict
    carries neither key: that row runs with the context's set."""
    v = dict(variant)
    given = {k: v.pop(k) for k in CRITIC_FIELDS if k in v}
    if not given:
        return v, None
    crit = dict(slope="wheels", w_orientation=0.0)
    crit.update(given)
    if crit["slope"] not in ("wheels", "body"):
        raise ValueError(f"slope must be 'wheels' or 'body', got {crit['slope']!r}")
    if not np.isfinite(F32(crit["w_orientation"])):
        raise ValueError(f"w_orientation must be finite, got {crit['w_orientation']!r}")
    return v, crit


SAMPLING_KEYS = ("antithetic", "nominal", "noise_beta")   # mppi_sampling (include/mppi.h) in a variant dict


def split_sampling(variant):
    """A variant dict that may carry the sampling keys -> (the dict without them, the sampling plan).

    "antithetic", "nominal" and "noise_beta" fill the batch's third table
    (mppi_batch_set_variant_sampling).  The plan is dict(antithetic=, nominal=, beta=) with the
    default for a key not given, or None when the dict carries none of the keys: that row runs with
    the controller's plan."""
    from .sampling import make_plan
    v = dict(variant)
    given = {k: v.pop(k) for k in SAMPLING_KEYS if k in v}
    if not given:
        return v, None
    return v, make_plan(given.get("antithetic", False), given.get("nominal", False), given.get("noise_beta", 0.0))


def variant_dict(proj="3d", **fields):
    """A full variant dict: the library's default parameters (_lib.make_params) and run()'s sigma
    schedule, overridden by `fields`."""
    base = dict(w_path=100.5, w_slope=50.5, w_speed=0.5, w_obstacle=25.0, collision_threshold=0.99,
                collision_penalty=100000.0, temperature=0.3, filter_k=3.5, filter_a=0.96, opt_filter_k=3.0,
                opt_filter_a=0.92, sigma_base=RUN_POLICY["sigma_base"], sigma_div=RUN_POLICY["sigma_div"])
    unknown = set(fields) - set(base)
    if unknown:
        raise ValueError(f"not fields of mppi_batch_variant: {sorted(unknown)}")
    base.update(fields)
    base["proj"] = proj
    return base


MAX_DEM_SLOTS, MAX_COSTMAP_SLOTS = 256, 1024    # kBatchMaxDems, kBatchMaxCostmaps (csrc/mppi_kernels.h)


def episode_scenes(E, K, dems=None, costmaps=None, episode_dem=None, episode_costmap=None,
                   episode_trajectories=None):
    """The per-episode scene arguments of MPPI_Controller.run_batch, checked and filled in:
    ([dem slot] * E, [costmap slot] * E, [K_e] * E) with -1 / -1 / 0 for the controller's own.

    dems / costmaps: the slots' contents (slot = list index); episode_dem / episode_costmap: E
    indices into them (-1 or None: the controller's); episode_trajectories: E counts in [1, K]
    (0 or None: K).  ValueError for a wrong length, an index without a table or outside it, too many
    slots, or a count outside [1, K].
    """
    def indices(name, idx, table, table_name, limit):
        n = 0 if table is None else len(table)
        if n > limit:
            raise ValueError(f"{table_name}: {n} slots, at most {limit}")
        out = [-1] * E if idx is None else [-1 if i is None else int(i) for i in idx]
        if len(out) != E:
            raise ValueError(f"{E} episodes but {len(out)} entries in {name}")
        if any(i >= 0 for i in out) and n == 0:
            raise ValueError(f"{name} names slots of `{table_name}`, which is empty")
        for e, i in enumerate(out):
            if i < -1 or i >= n:
                raise ValueError(f"{name}[{e}] = {i} outside the {n} slots of `{table_name}`")
        return out

    ed = indices("episode_dem", episode_dem, dems, "dems", MAX_DEM_SLOTS)
    ec = indices("episode_costmap", episode_costmap, costmaps, "costmaps", MAX_COSTMAP_SLOTS)
    ek = [0] * E if episode_trajectories is None else [0 if k is None else int(k) for k in episode_trajectories]
    if len(ek) != E:
        raise ValueError(f"{E} episodes but {len(ek)} entries in episode_trajectories")
    for e, k in enumerate(ek):
        if k != 0 and not 1 <= k <= int(K):
            raise ValueError(f"episode_trajectories[{e}] = {k} outside [1, {int(K)}]")
    return ed, ec, ek


def campaign_tasks(N, K, max_loops, variants=None, dems=None, costmaps=None, task_variant=None, task_dem=None,
                   task_costmap=None, task_trajectories=None):
    """The per-task arguments of MPPI_Controller.run_campaign, checked and filled in:
    ([variant row] * N, [dem slot] * N, [costmap slot] * N, [K_i] * N, [max_steps] * N), with
    -1 / -1 / -1 / 0 for the controller's own.

    The checks of episode_scenes with tasks in place of episodes, and: task_variant[i] an index into
    `variants` (-1 or None: none); max_loops one step cap >= 1 for every task, or N of them.
    ValueError names the argument and the task.
    """
    N = int(N)
    if N < 1:
        raise ValueError("a campaign needs at least one task")
    try:
        ed, ec, ek = episode_scenes(N, K, dems, costmaps, task_dem, task_costmap, task_trajectories)
    except ValueError as err:
        raise ValueError(str(err).replace("episode_", "task_").replace("episodes", "tasks")) from None
    nv = 0 if variants is None else len(variants)
    tv = [-1] * N if task_variant is None else [-1 if v is None else int(v) for v in task_variant]
    if len(tv) != N:
        raise ValueError(f"{N} tasks but {len(tv)} entries in task_variant")
    if any(v >= 0 for v in tv) and nv == 0:
        raise ValueError("task_variant names rows of `variants`, which is empty")
    for i, v in enumerate(tv):
        if v < -1 or v >= nv:
            raise ValueError(f"task_variant[{i}] = {v} outside the {nv} rows of `variants`")
    caps = [int(max_loops)] * N if np.ndim(max_loops) == 0 else [int(m) for m in max_loops]
    if len(caps) != N:
        raise ValueError(f"{N} tasks but {len(caps)} entries in max_loops")
    for i, m in enumerate(caps):
        if m < 1:
            raise ValueError(f"max_loops[{i}] = {m}: a task's step cap must be >= 1")
    return tv, ed, ec, ek, caps


def campaign_makespan(lengths, lanes):
    """The batch steps a campaign needs for tasks that take `lengths` steps on `lanes` lanes: the
    device's claim rule, greedy list scheduling in list order.  A free lane takes the next task of
    the list in the same step; a task of length 0 (its start inside the goal tolerance) is consumed
    without a step.  Plain Python."""
    lanes = int(lanes)
    if lanes < 1:
        raise ValueError("lanes must be >= 1")
    todo = [int(n) for n in lengths]
    if any(n < 0 for n in todo):
        raise ValueError("lengths must be >= 0")
    todo.reverse()
    busy = []          # steps left of each running lane

    def fill():
        while len(busy) < lanes and todo:
            n = todo.pop()
            if n > 0:
                busy.append(n)

    fill()
    steps = 0
    while busy:
        steps += 1
        busy[:] = [n - 1 for n in busy if n > 1]
        fill()
    return steps


LENGTH_STRIDE = 5    # compute_length samples every fifth waypoint (evaluate_trajectory.py:43-53)


def path_length(rows):
    """compute_length of evaluate_trajectory.py:43-53 on logged waypoints, in float64: the `length` of
    a scored task list (mppi_batch_get_task_scores).  rows: [L, >= 3] float32, x, y, z first (a task
    log).  Over the sampled rows 0, 5, 10, ... < L: for consecutive sampled rows a -> b, each
    difference of the float32 coordinates widened first, d = sqrt((dx dx + dy dy) + dz dz), summed in
    row order.  Fewer than two sampled rows give 0."""
    rows = np.asarray(rows, dtype=F32)
    p = rows.reshape(len(rows), rows.shape[-1] if rows.ndim > 1 else 3)[::LENGTH_STRIDE, :3].astype(np.float64)
    length = np.float64(0.0)
    for a, b in zip(p[:-1], p[1:]):
        dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        length = length + np.sqrt((dx * dx + dy * dy) + dz * dz)
    return length


def dm_atan2(y, x):
    """The deterministic float64 arctangent of csrc/mppi_detmath.h (dm_atan2), the same IEEE operations in
    the same order, so a device result equals this bit for bit.  Arrays or scalars (broadcast), finite.

    t = min(|y|, |x|) / max(|y|, |x|) (0 for y = x = 0); three half-angle steps t <- t / (1 + sqrt(1 + t t));
    the 12-term odd series in Horner form over z = t t, times t, times 8; |y| > |x|: pi/2 - r; x < 0:
    pi - r; y < 0: -r.  A signed zero counts as +0."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    y, x = np.broadcast_arrays(y, x)
    ay = np.where(y < 0.0, -y, y)
    ax = np.where(x < 0.0, -x, x)
    small = ay < ax
    mn = np.where(small, ay, ax)
    mx = np.where(small, ax, ay)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(mx > 0.0, mn / np.where(mx > 0.0, mx, 1.0), 0.0)
    for _ in range(3):
        t = t / (1.0 + np.sqrt(1.0 + t * t))
    z = t * t
    p = np.full(z.shape, -1.0 / 23.0)
    for c in (1.0 / 21.0, -1.0 / 19.0, 1.0 / 17.0, -1.0 / 15.0, 1.0 / 13.0, -1.0 / 11.0, 1.0 / 9.0, -1.0 / 7.0,
              1.0 / 5.0, -1.0 / 3.0, 1.0):
        p = p * z + c
    r = (t * p) * 8.0
    r = np.where(ay > ax, 1.5707963267948966 - r, r)
    r = np.where(x < 0.0, 3.141592653589793 - r, r)
    r = np.where(y < 0.0, -r, r)
    return r if r.ndim else np.float64(r)


METRICS_STRIDE = 20                  # compute_path_metrics' k (MPPI_isaac.py:236)
METRICS_FIELDS = ("length20", "angle_up", "angle_down", "distance_up")     # mppi_path_metrics
DEGREES = 57.29577951308232          # 180 / pi, np.degrees' factor


def path_metrics(rows):
    """compute_path_metrics of MPPI_isaac.py:231-256 (k = 20) on logged waypoints, in float64: the
    `metrics` of a scored task list, a tracked run or Batch.score(metrics=True), bit for bit
    (csrc/mppi_path_metrics.h is the device's statement).  rows: [L, >= 3] float32, x, y, z first.

    Segments m = 0, 1, ... while 20 m + 21 < L: s = p[20 m + 21] - p[20 m], the float32 coordinates
    widened first (the reference's p[i + 20] - p[i - 1] over i = 1, 21, ... < L - 20; neighbours overlap
    by one row).  hh = s.x s.x + s.y s.y, n = sqrt(hh + s.z s.z); length20 += n; if n > 0:
    a = dm_atan2(s.z, sqrt(hh)) (180 / pi), added to angle_up if a > 0, else |a| to angle_down; if
    s.z > 0: distance_up += s.z.  Sums in row order.  Returns float64 [4] in METRICS_FIELDS order;
    fewer than 22 rows give zeros."""
    rows = np.asarray(rows, dtype=F32)
    L = len(rows)
    p = rows.reshape(L, rows.shape[-1] if rows.ndim > 1 else 3)[:, :3].astype(np.float64)
    length = up = down = climbed = np.float64(0.0)
    k = METRICS_STRIDE
    for i in range(0, L - k - 1, k):
        s = p[i + k + 1] - p[i]
        hh = s[0] * s[0] + s[1] * s[1]
        n = np.sqrt(hh + s[2] * s[2])
        length = length + n
        if n > 0.0:
            a = dm_atan2(s[2], np.sqrt(hh)) * DEGREES
            if a > 0.0:
                up = up + a
            else:
                down = down + np.abs(a)
        if s[2] > 0.0:
            climbed = climbed + s[2]
    return np.array([length, up, down, climbed], dtype=np.float64)


SUMMARY_FIELDS = ("cost", "path", "slope", "speed", "obstacle", "length")


def campaign_summary(results, by=None):
    """The table of a campaign, per group of tasks: what the thesis's stats_results.py prints per
    controller variant.  Plain numpy, no GPU.

    results: one dict per task with `reached`, `cost`, `terms` (4 values: path, slope, speed,
    obstacle), `collisions` and `length`: MPPI_Controller.run_campaign(..., score=...) returns them
    (its per-task dicts and the score arrays; see `campaign_results`).  by: one group key per task
    (task_variant, say); None: one group, keyed None.

    results may also be the stacked rows of tracked runs (Batch.runs() / BatchStepper.runs(): a dict of
    arrays with an `episode` column); `by` is then one key per episode (the variant each rover of
    the simulator ran with, say), and the rows are taken through tracked_results first.

    Returns {key: dict(count, reached, collided (runs with at least one collision), mean=dict(cost,
    path, slope, speed, obstacle, length), std=the same fields)} in float64, the standard deviation
    the population's (numpy's default), keys in order of first appearance.  When every result carries
    `metrics` (4 values in METRICS_FIELDS order: the runs were scored with metrics=True), mean and std
    also hold length20, angle_up, angle_down and distance_up."""
    if isinstance(results, dict):
        results, by = tracked_results(results, by)
    results = list(results)
    keys = [None] * len(results) if by is None else list(by)
    if len(keys) != len(results):
        raise ValueError(f"{len(results)} results but {len(keys)} group keys")
    groups = {}
    for k, r in zip(keys, results):
        groups.setdefault(k, []).append(r)
    out = {}
    for k, rs in groups.items():
        terms = np.asarray([np.asarray(r["terms"], np.float64).reshape(4) for r in rs])
        cols = dict(cost=np.asarray([r["cost"] for r in rs], np.float64), path=terms[:, 0], slope=terms[:, 1],
                    speed=terms[:, 2], obstacle=terms[:, 3], length=np.asarray([r["length"] for r in rs], np.float64))
        fields = SUMMARY_FIELDS
        if all(r.get("metrics") is not None for r in rs):
            met = np.asarray([np.asarray(r["metrics"], np.float64).reshape(4) for r in rs])
            cols.update({f: met[:, j] for j, f in enumerate(METRICS_FIELDS)})
            fields = SUMMARY_FIELDS + METRICS_FIELDS
        out[k] = dict(count=len(rs), reached=sum(1 for r in rs if r["reached"]),
                      collided=sum(1 for r in rs if int(r["collisions"]) > 0),
                      mean={f: float(np.mean(cols[f])) for f in fields},
                      std={f: float(np.std(cols[f])) for f in fields})
    return out


RUN_STATUS = {0: "none", 1: "reached", 2: "cap", 3: "abandoned"}     # mppi_batch_get_runs' status


def tracked_results(runs, by=None, abandoned=False):
    """The stacked rows of tracked runs (Batch.runs(): dict of arrays with `episode`, `status`, `reached`,
    `cost`, `terms`, `collisions`, `length`, ...) as (the per-run dicts campaign_summary takes, one group
    key per run).  Rows no run has ended into (status 0) are left out, and abandoned runs (status 3:
    cut short by a reset) unless abandoned=True; by: one key per episode (None: every run keyed None)."""
    ep = np.asarray(runs["episode"], np.int64)
    status = np.asarray(runs["status"], np.int64)
    if by is not None:
        by = list(by)
        if len(ep) and int(ep.max()) >= len(by):
            raise ValueError(f"{int(ep.max()) + 1} episodes but {len(by)} group keys")
    keep = [i for i in range(len(ep)) if status[i] in ((1, 2, 3) if abandoned else (1, 2))]
    out = [dict(episode=int(ep[i]), run=int(runs["run"][i]), status=int(status[i]), reached=bool(runs["reached"][i]),
                loops=int(runs["steps"][i]), cost=runs["cost"][i], terms=runs["terms"][i],
                collisions=runs["collisions"][i], length=runs["length"][i],
                **({"metrics": runs["metrics"][i]} if "metrics" in runs else {})) for i in keep]
    return out, [None if by is None else by[int(ep[i])] for i in keep]


def campaign_results(tasks, scores):
    """run_campaign's (per-task dicts, score arrays) as the per-task dicts campaign_summary takes:
    each task's dict with its cost, terms, collisions and length added."""
    return [dict(t, cost=scores["cost"][i], terms=scores["terms"][i], collisions=scores["collisions"][i],
                 length=scores["length"][i], **({"metrics": scores["metrics"][i]} if "metrics" in scores else {}))
            for i, t in enumerate(tasks)]


def normalise_heading(hv):
    """Row 0 of heading_sim widened to float64 and divided by sqrt((h0 h0 + h1 h1) + h2 h2) (the sum
    left to right, every operation rounded once), each component rounded to float32."""
    h = np.asarray(hv, dtype=F32).astype(np.float64)
    n = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    return np.array([h[0] / n, h[1] / n, h[2] / n], dtype=np.float64).astype(F32)


def is_active(state, policy=None):
    """The loop's condition before a step: not (|x - goal_x| <= tol and |y - goal_y| <= tol), in
    float32; a NaN coordinate is never inside the tolerance."""
    tol = F32((policy or RUN_POLICY)["goal_tol"])
    x, y = F32(state["x"]), F32(state["y"])
    gx, gy = F32(state["goal_x"]), F32(state["goal_y"])
    return not bool(np.abs(x - gx) <= tol and np.abs(y - gy) <= tol)


def advance_state(state, traj0, heading0, v, w, robot_radius, policy=None):
    """The state after one closed-loop step.

    traj0, heading0: row 0 of the optimal rollout (traj_sim[0], heading_sim[0]); v, w: element 0 of
    the filtered optimal velocities; robot_radius: params.robot_radius; policy: dict(sigma_base,
    sigma_div, goal_tol), default run()'s.  Returns (new state dict, log row [8] float32: x, y, z,
    the normalised heading, v, w).  Every value is float32; the goal is unchanged.
    """
    pol = policy or RUN_POLICY
    base, div = F32(pol["sigma_base"]), F32(pol["sigma_div"])
    t = np.asarray(traj0, dtype=F32)
    v, w, r = F32(v), F32(w), F32(robot_radius)
    h = normalise_heading(heading0)
    ww = F32(F32(w * w) / div)
    half = F32(F32(w * r) / F32(2.0))
    new = dict(
        x=t[0], y=t[1], heading=h,
        left_wheel_speed=F32(v - half), right_wheel_speed=F32(v + half),
        goal_x=F32(state["goal_x"]), goal_y=F32(state["goal_y"]),
        std_dev_u1=np.maximum(base, F32(base - ww)), std_dev_u2=np.maximum(base, F32(base + ww)))
    row = np.array([t[0], t[1], t[2], h[0], h[1], h[2], v, w], dtype=F32)
    return new, row


def state_dict(x, y, heading=(1.0, 0.0, 0.0), left_wheel_speed=0.0, right_wheel_speed=0.0, goal_x=0.0,
               goal_y=0.0, std_dev_u1=0.25, std_dev_u2=0.25):
    """A state dict in float32, the heading used as given."""
    return dict(x=F32(x), y=F32(y), heading=np.asarray(heading, dtype=F32).copy(),
                left_wheel_speed=F32(left_wheel_speed), right_wheel_speed=F32(right_wheel_speed),
                goal_x=F32(goal_x), goal_y=F32(goal_y), std_dev_u1=F32(std_dev_u1), std_dev_u2=F32(std_dev_u2))


STATE_WIDTH = 11    # floats of mppi_state: the row of Batch.step_device's `states`


def pack_states(states):
    """State dicts -> float32 [E, 11], the rows Batch.step_device reads: x, y, heading[3],
    left_wheel_speed, right_wheel_speed, goal_x, goal_y, std_dev_u1, std_dev_u2 (mppi_state's field
    order; the heading as given).  Upload it once, then keep the rows current on the device."""
    out = np.zeros((len(states), STATE_WIDTH), dtype=F32)
    for e, s in enumerate(states):
        h = np.asarray(s["heading"], dtype=F32).reshape(3)
        out[e] = (s["x"], s["y"], h[0], h[1], h[2], s["left_wheel_speed"], s["right_wheel_speed"],
                  s["goal_x"], s["goal_y"], s["std_dev_u1"], s["std_dev_u2"])
    return out


def unpack_states(rows):
    """The inverse of pack_states: float32 [E, 11] -> list of state dicts."""
    rows = np.asarray(rows, dtype=F32)
    if rows.ndim != 2 or rows.shape[1] != STATE_WIDTH:
        raise ValueError(f"states must have shape (E, {STATE_WIDTH}), got {rows.shape}")
    return [state_dict(r[0], r[1], r[2:5], r[5], r[6], r[7], r[8], r[9], r[10]) for r in rows]


def to_mppi_state(state):
    """The ctypes MppiState of a state dict (the heading as given, no renormalisation)."""
    from . import _lib
    s = _lib.MppiState()
    s.x, s.y = float(state["x"]), float(state["y"])
    for i in range(3):
        s.heading[i] = float(state["heading"][i])
    s.left_wheel_speed = float(state["left_wheel_speed"])
    s.right_wheel_speed = float(state["right_wheel_speed"])
    s.goal_x, s.goal_y = float(state["goal_x"]), float(state["goal_y"])
    s.std_dev_u1, s.std_dev_u2 = float(state["std_dev_u1"]), float(state["std_dev_u2"])
    return s


def from_mppi_state(s):
    """The state dict of a ctypes MppiState."""
    return state_dict(s.x, s.y, [s.heading[0], s.heading[1], s.heading[2]], s.left_wheel_speed,
                      s.right_wheel_speed, s.goal_x, s.goal_y, s.std_dev_u1, s.std_dev_u2)
