"""GPU: wheel contacts, the wheel form of the slope critic and the path metrics of executed paths
(include/mppi.h mppi_batch_set_wheel_log / _score_ex / _set_score_options).

  1. own model: every wheel-log row is left_wheel_sim[0] | right_wheel_sim[0] of the single-context step
     (a fresh Engine stepped from the host, and the CPU oracle for one episode), bit for bit, under both
     projections; log rows, states and nominal sequences are those of the batch without the wheel log.
  2. Batch.score(slope="wheels") and the path metrics after the run: Engine.score_paths on a wheels-mode
     context fed the fetched logs, bit for bit, for path lengths 0, 1, 3, 4, 5, 6 and 45; both
     path-follow branches, a costmap slot, another yardstick; oracle.mppi_ref.critics for a short path.
  3. a scored list with the wheel mode and the metrics on: scores and metrics are those of the
     after-the-run call on a logged twin, on 1 and 3 lanes, with and without a log.
  4. tracked steps with a synthetic plant: the wheel rows are the rollout's rule restated from the
     oracle's primitives, the run's score is Batch.score(slope="wheels") of the kept log, the metrics are
     mppi_amd.batch.path_metrics of the same rows; an abandoned run, resets and `done` as before.
  5. off means untouched, and the refusals.
K = 256, H = 20, helpers.c3_scene().
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V
import test_gpu_batch_step_device as S

pytestmark = pytest.mark.gpu

F32 = np.float32
K, H = 256, 20
FAR = (65.0, 10.0)
MPPI_EINVAL, MPPI_ESTATE = -1, -3
HORIZON = 0.045 * 2.0 * H
# the issue's three starts: from them the wheel and the body form of the slope term differ
STARTS = [(-60.0, -5.0), (-20.0, -18.0), (10.0, 12.0)]
INSIDE = B.MAIN[3][:3]
NEAR = B.MAIN[0][:3]
_bits = S._bits


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _policy():
    from mppi_amd import _lib
    return _lib.make_policy(**B.RUN)


def _set(batch, episodes, **kw):
    for e, (start, goal, seed) in enumerate(episodes):
        batch.set_episode(e, V.mppi_state(B.start_state(start, goal)), seed, **{k: v[e] for k, v in kw.items()})


def _origins(episodes):
    return [V.origin_state(s[0], s[1], g[0], g[1]) for s, g, _ in episodes]


def engine_wheel_loop(start, goal, seed, n_steps, proj):
    """batch_refs.engine_loop's pattern, keeping row 0 of the wheel paths of every step: (result, wheel
    rows [n, 6])."""
    from helpers import c3_scene
    from mppi_amd import _lib
    Z, hw, cm = c3_scene()
    st = B.start_state(start, goal)
    eng = _lib.Engine(_lib.make_params(K, H, seed=seed), 0)
    try:
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        r = float(eng.params.robot_radius)
        rows, wheels = [], []
        i = 0
        while i < n_steps and B.active(st, B.RUN):
            eng.set_state(_lib.make_state(st["x"], st["y"], st["heading"], st["wl"], st["wr"], st["gx"], st["gy"],
                                          st["s1"], st["s2"]))
            o = eng.step(proj, i)
            wheels.append(np.concatenate([np.asarray(o["left_wheel_sim"], F32).reshape(-1, 3)[0],
                                          np.asarray(o["right_wheel_sim"], F32).reshape(-1, 3)[0]]))
            st, row = B.rule(st, o["traj_sim"][0], o["heading_sim"][0], o["lin_vel"][0], o["ang_vel"][0], r, B.RUN)
            rows.append(row)
            i += 1
        u1, u2 = eng.get_nominal()
    finally:
        eng.close()
    return B._result(rows, st, u1, u2, i, B.RUN), np.asarray(wheels, F32).reshape(-1, 6)


def oracle_wheel_loop(start, goal, seed, n_steps, proj):
    """batch_refs.oracle_loop keeping lw_sim[0] | rw_sim[0] of every step."""
    from helpers import c3_scene, oracle_scene
    from oracle import mppi_ref as R
    scene = oracle_scene(*c3_scene())
    p = dataclasses.replace(R.Params(), K=K, H=H, seed=seed)
    st = B.start_state(start, goal)
    u1, u2 = np.zeros(H, F32), np.zeros(H, F32)
    wheels = []
    for i in range(n_steps):
        s = R.State(x=float(st["x"]), y=float(st["y"]), heading=np.asarray(st["heading"], np.float64),
                    left_wheel_speed=float(st["wl"]), right_wheel_speed=float(st["wr"]), goal_x=float(st["gx"]),
                    goal_y=float(st["gy"]), std_dev_u1=float(st["s1"]), std_dev_u2=float(st["s2"]))
        o = R.mppi_step(p, scene, s, u1, u2, i, proj)
        u1, u2 = o["u1_opt"], o["u2_opt"]
        wheels.append(np.concatenate([o["lw_sim"][0], o["rw_sim"][0]]).astype(F32))
        st, _ = B.rule(st, o["traj_sim"][0], o["hv_sim"][0], o["v_opt"][0], o["w_opt"][0], p.robot_radius, B.RUN)
    return np.asarray(wheels, F32)


def score_wheels(engine, rows, wheels, origin):
    """Engine.score_paths on one logged path with its two contact paths (a context in the wheels mode)."""
    if len(rows) == 0:
        return dict(cost=F32(0), terms=np.zeros(4, F32), collisions=np.int32(0))
    assert engine.critics()["slope"] == "wheels"
    r = engine.score_paths(np.ascontiguousarray(rows[None, :, 0:3]), np.ascontiguousarray(rows[None, :, 6]),
                           np.ascontiguousarray(wheels[None, :, 0:3]), np.ascontiguousarray(wheels[None, :, 3:6]),
                           lengths=np.array([len(rows)], np.int32), state=origin)
    return dict(cost=r["cost"][0], terms=r["terms"][0], collisions=r["collisions"][0])


def check_wheel_scores(got, engine, logs, wlogs, origins, tag):
    for e in range(len(logs)):
        want = score_wheels(engine, logs[e], wlogs[e], origins[e])
        assert got["rows"][e] == len(logs[e]), (tag, e)
        assert _bits(got["cost"][e]) == _bits(F32(want["cost"])), (tag, e, got["cost"][e], want["cost"])
        assert np.array_equal(_bits(got["terms"][e]), _bits(np.asarray(want["terms"], F32))), \
            (tag, e, got["terms"][e], want["terms"])
        assert got["collisions"][e] == want["collisions"], (tag, e)


def check_metrics(got, logs, tag):
    from mppi_amd.batch import path_metrics
    want = np.array([path_metrics(r) for r in logs], np.float64).reshape(len(logs), 4)
    assert got.shape == want.shape and got.dtype == np.float64, tag
    assert np.array_equal(_bits64(got), _bits64(want)), (tag, got, want)


# ---- 1. own model, plain batch ----
@functools.lru_cache(maxsize=None)
def _ref45(e, proj):
    return engine_wheel_loop(STARTS[e], FAR, 11 + e, 45, proj)


@pytest.mark.parametrize("proj", ["3d", "2d"])
def test_wheel_log_rows_are_the_single_context_steps(proj):
    S._gpu()
    from mppi_amd import _lib
    eps = [(s, FAR, 11 + e) for e, s in enumerate(STARTS)]
    eng = V.make_engine(K, H)
    try:
        for n in (6, 45):
            plain = _lib.Batch(eng, len(eps))
            _set(plain, eps)
            plain.run(n, proj, _policy())
            batch = _lib.Batch(eng, len(eps))
            batch.set_wheel_log()
            _set(batch, eps)
            batch.run(n, proj, _policy())
            for e in range(len(eps)):
                ref, wheels = _ref45(e, proj)
                got = batch.wheel_log(e)
                assert got.shape == (n, 6)
                assert np.array_equal(_bits(got), _bits(wheels[:n])), f"wheel rows of {e}, {proj}, {n} steps"
                assert np.array_equal(_bits(batch.log(e)), _bits(ref["rows"][:n])), f"log rows of {e}"
                V.same(V.collect(batch, e), V.collect(plain, e), f"episode {e} with and without the wheel log")
                assert np.array_equal(_bits(batch.wheel_log(e, 2, 3)), _bits(wheels[2:5]))
            if proj == "3d":
                assert np.abs(batch.wheel_log(0)).min(axis=0).max() > 0     # contacts, not zeros
            plain.close()
            batch.close()
    finally:
        eng.close()


@pytest.mark.parametrize("proj", ["3d", "2d"])
def test_wheel_log_rows_are_the_oracles(proj):
    S._gpu()
    from mppi_amd import _lib
    want = oracle_wheel_loop(STARTS[1], FAR, 12, 6, proj)
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 1)
        batch.set_wheel_log()
        _set(batch, [(STARTS[1], FAR, 12)])
        batch.run(6, proj, _policy())
        got = batch.wheel_log(0)
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
        batch.close()
    finally:
        eng.close()


# ---- 2. the wheel score and the metrics after the run ----
def test_wheel_score_after_the_run():
    S._gpu()
    from mppi_amd import _lib
    from mppi_amd.batch import variant_dict
    eps = [(s, FAR, 21 + e) for e, s in enumerate(STARTS)] + [NEAR, INSIDE]
    other = dict(w_path=3.0, w_slope=7.0, w_speed=11.0, w_obstacle=0.25, collision_threshold=0.5,
                 collision_penalty=1000.0)
    origins = _origins(eps)
    eng = V.make_engine(K, H)
    eng2 = V.make_engine(K, H, **other)
    try:
        batch = _lib.Batch(eng, len(eps))
        batch.set_wheel_log()
        seen = set()
        for cap in (1, 3, 4, 5, 6, 45):
            _set(batch, eps)
            batch.run(cap, "3d", _policy())
            logs = [batch.log(e) for e in range(len(eps))]
            wlogs = [batch.wheel_log(e) for e in range(len(eps))]
            assert all(len(w) == len(r) for w, r in zip(wlogs, logs))
            seen |= {len(r) for r in logs}
            got = batch.score(slope="wheels", metrics=True)
            check_wheel_scores(got, eng, logs, wlogs, origins, f"cap {cap}")
            check_metrics(got["metrics"], logs, f"cap {cap}")
            body = batch.score()
            V.check_scores(body, eng, logs, origins, f"body, cap {cap}")
            again = batch.score(slope="body", metrics=True)
            for k in ("cost", "terms", "collisions", "rows"):
                assert np.array_equal(again[k], body[k]), k
            for k in (0, 2, 3):       # everything but the slope term is the body form's
                assert np.array_equal(_bits(got["terms"][:, k]), _bits(body["terms"][:, k])), (cap, k)
            if cap == 45:
                print("slope, wheels:", got["terms"][:3, 1], "body:", body["terms"][:3, 1])
                assert (got["terms"][:3, 1] != body["terms"][:3, 1]).any()
                assert got["metrics"][:3, 0].all()
                got2 = batch.score(yardstick=variant_dict("3d", **other), slope="wheels")
                check_wheel_scores(got2, eng2, logs, wlogs, origins, "yardstick")
                assert not np.array_equal(got2["cost"], got["cost"])
            if cap == 5:              # a short path against the oracle's critics, each term on its own
                for e in (0, 1):
                    terms, col = _oracle_wheel_terms(logs[e], wlogs[e], eps[e][0], eps[e][1])
                    assert np.array_equal(_bits(got["terms"][e]), _bits(terms)), (e, got["terms"][e], terms)
                    assert got["collisions"][e] == col
        assert {0, 1, 3, 4, 5, 6, 45} <= seen, seen
        near_rows = len(batch.log(3))
        assert 0 < near_rows < 45                  # the near path-follow branch, ended by the goal test
        batch.close()
    finally:
        eng2.close()
        eng.close()


def _oracle_wheel_terms(rows, wheels, origin_xy, goal):
    from helpers import c3_scene
    from oracle import mppi_ref as R
    Z, hw, cm = c3_scene()
    sc = R.Scene(Z, hw, cm)
    traj = np.ascontiguousarray(rows[None, :, 0:3], dtype=F32)
    lw = np.ascontiguousarray(wheels[None, :, 0:3], dtype=F32)
    rw = np.ascontiguousarray(wheels[None, :, 3:6], dtype=F32)
    v = np.ascontiguousarray(rows[None, :, 6], dtype=F32)
    p = R.Params(K=1, H=len(rows), horizon=HORIZON)
    st = R.State(x=float(origin_xy[0]), y=float(origin_xy[1]), goal_x=float(goal[0]), goal_y=float(goal[1]))
    terms = np.stack([R.critics(dataclasses.replace(p, **{w: (1.0 if w == one else 0.0) for w in V.WEIGHTS}),
                                sc, st, traj, lw, rw, v) for one in V.WEIGHTS], -1)[0].astype(F32)
    col = int((R.costmap_at(sc, traj[:, :, 0], traj[:, :, 1]) > p.f("collision_threshold")).sum())
    return terms, col


def test_wheel_score_on_a_costmap_slot():
    """An episode that holds a costmap slot is scored on it in the wheel form too: a reference engine whose
    own costmap is the slot's."""
    S._gpu()
    from helpers import c3_scene
    from mppi_amd import _lib
    Z, hw, cm = c3_scene()
    cm2 = np.ascontiguousarray(np.clip(cm[::-1, ::-1] + F32(0.25), 0, 1).astype(F32))
    eps = [(STARTS[0], FAR, 31), (STARTS[0], FAR, 31)]
    eng = V.make_engine(K, H)
    eng_cm = S._engine(K, cm=cm2)
    try:
        batch = _lib.Batch(eng, 2)
        batch.set_wheel_log()
        batch.set_costmap(0, cm2)
        _set(batch, eps, costmap=[-1, 0])
        batch.run(7, "3d", _policy())
        logs = [batch.log(e) for e in range(2)]
        wlogs = [batch.wheel_log(e) for e in range(2)]
        got = batch.score(slope="wheels")
        o = _origins(eps)
        check_wheel_scores(dict((k, v[:1]) for k, v in got.items()), eng, logs[:1], wlogs[:1], o[:1], "context")
        check_wheel_scores(dict((k, v[1:]) for k, v in got.items()), eng_cm, logs[1:], wlogs[1:], o[1:], "slot")
        assert got["terms"][0, 3] != got["terms"][1, 3]
        batch.close()
    finally:
        eng_cm.close()
        eng.close()


# ---- 3. online equals after the run ----
def far(seed, start=STARTS[0]):
    return (start, FAR, seed)


# caps 21, 22, 23, 42, 43: one row before, at and after the first and the second segment of the metrics;
# 1 .. 4: the boundaries of the slope chain; a zero-step task and a near-goal one in between
LIST = [(far(1), 21), (INSIDE, 5), (far(2, STARTS[1]), 22), (far(3), 1), (far(4, STARTS[2]), 23), (NEAR, 40), (far(5), 2),
        (far(6, STARTS[1]), 42), (far(7), 3), (far(8, STARTS[2]), 43), (far(9), 4)]


def _tasks():
    from mppi_amd import _lib
    return [_lib.make_task(V.mppi_state(B.start_state(start, goal)), seed, cap) for (start, goal, seed), cap in LIST]


def _run_list(batch):
    done, calls = 0, 0
    while done < len(LIST):
        done, _ = batch.run_tasks(100000, "3d", _policy())
        calls += 1
        assert calls < 100


@functools.lru_cache(maxsize=None)
def _twin():
    """The logged twin: a plain list with the wheel log on, scored after the run."""
    S._gpu()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 3)
        batch.set_wheel_log()
        batch.set_tasks(_tasks())
        _run_list(batch)
        n = len(LIST)
        logs = [batch.task_log(i) for i in range(n)]
        wlogs = [batch.task_wheel_log(i) for i in range(n)]
        after = batch.score_tasks(slope="wheels", metrics=True)
        body = batch.score_tasks()
        origins = [V.origin_state(s[0], s[1], g[0], g[1]) for (s, g, _), _ in LIST]
        check_wheel_scores(after, eng, logs, wlogs, origins, "twin")
        check_metrics(after["metrics"], logs, "twin")
        batch.close()
    finally:
        eng.close()
    return dict(logs=logs, wlogs=wlogs, after=after, body=body)


def test_twin_covers_the_cases():
    t = _twin()
    rows = [len(r) for r in t["logs"]]
    assert {0, 1, 2, 3, 4, 21, 22, 23, 42, 43} <= set(rows), rows
    m = t["after"]["metrics"]
    for i, n in enumerate(rows):
        assert bool(m[i, 0] > 0) == (n >= 22), (i, n, m[i])
    assert (t["after"]["terms"][:, 1] != t["body"]["terms"][:, 1]).any()
    for k in (0, 2, 3):
        assert np.array_equal(_bits(t["after"]["terms"][:, k]), _bits(t["body"]["terms"][:, k]))


@pytest.mark.parametrize("keep_log", [True, False])
@pytest.mark.parametrize("lanes", [1, 3])
def test_online_wheel_scores_and_metrics_are_the_after_the_run_ones(lanes, keep_log):
    t = _twin()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, lanes)
        batch.set_tasks(_tasks(), scored=dict(slope="wheels", metrics=True), keep_log=keep_log)
        _run_list(batch)
        got = batch.task_scores()
        want = t["after"]
        for k in ("cost", "terms"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, got[k], want[k])
        for k in ("collisions", "rows"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(_bits64(got["metrics"]), _bits64(want["metrics"])), (got["metrics"], want["metrics"])
        if keep_log:
            for i in range(len(LIST)):
                assert np.array_equal(_bits(batch.task_log(i)), _bits(t["logs"][i])), i
            with pytest.raises(RuntimeError, match="wheel log"):      # the wheel log was not on for this list
                batch.task_wheel_log(0, 0, 1)
        # metrics only (the body form of the slope term stays): the existing scored list's scores
        batch.set_tasks(_tasks(), scored=dict(metrics=True), keep_log=False)
        _run_list(batch)
        got = batch.task_scores()
        assert np.array_equal(_bits(got["terms"]), _bits(t["body"]["terms"]))
        assert np.array_equal(_bits(got["cost"]), _bits(t["body"]["cost"]))
        assert np.array_equal(_bits64(got["metrics"]), _bits64(want["metrics"]))
        batch.close()
    finally:
        eng.close()


# ---- 4. tracked steps with a synthetic plant ----
def _contacts(sc, x, y, h, off):
    """projection_warp.py:331-347 restated from the oracle's primitives: the contacts of pose (x, y, h)."""
    from oracle import mppi_ref as R
    x, y = np.array([x], F32), np.array([y], F32)
    hv = tuple(np.array([c], F32) for c in h)
    q = R.get_corners_heights(sc, x, y)
    n = R.normal_on_grid(q, sc.res)
    cr = R.cross3(n, hv)
    r = (off * cr[0], off * cr[1])
    out = []
    for sign in (1, -1):
        xw = x + r[0] if sign > 0 else x - r[0]
        yw = y + r[1] if sign > 0 else y - r[1]
        i, j = R.dem_cell(sc, xw, yw)
        out += [xw[0], yw[0], R.dem_at(sc, j, i)[0]]
    return np.array(out, F32)


def _plant(n):
    """Poses [n, 2, 11] and heights [n, 2] no model produced: a walk through the origin (negative and
    positive coordinates), row 21 = row 0 (a repeated pose: a zero-length metrics segment), rows 20 and 41
    at one height (a level segment), one pose in the map's corner, headings with a z component that are
    not tangent to the surface."""
    rng = np.random.default_rng(77)
    t = np.zeros((n, 2, 11), F32)
    z = np.zeros((n, 2), F32)
    for e in range(2):
        for i in range(n):
            a = 0.13 * i + e
            x = -2.0 + 0.1 * i + 0.3 * np.sin(a)
            y = -1.5 + 0.07 * i + (0.4 * e)
            h = np.array([np.cos(a) * 0.8, np.sin(a) * 0.8, 0.6])
            t[i, e] = (x, y, h[0], h[1], h[2], rng.uniform(0, 1), rng.uniform(0, 1), FAR[0], FAR[1], 0.3, 0.3)
            z[i, e] = 0.5 + 0.02 * i * np.cos(0.2 * i)
        t[8, e, 0:2] = (-74.97, 74.96) if e == 0 else (74.98, -74.95)      # a map corner
    # ingest i makes row i - 1
    t[22, :, 0:5] = t[1, :, 0:5]
    z[22] = z[1]
    z[42] = z[21]
    return t, z


def test_tracked_ingest_with_a_synthetic_plant():
    torch = S._gpu()
    from helpers import c3_scene
    from mppi_amd import _lib
    from mppi_amd.batch import path_metrics
    from oracle import mppi_ref as R
    Z, hw, cm = c3_scene()
    Z1 = np.ascontiguousarray(Z[::-1, ::-1])
    n, cap, seeds = 47, 45, (61, 62)
    t, z = _plant(n)
    reset_at = 30       # episode 1 is reset there: its run of 29 rows is abandoned
    off = F32(0.2)
    eng = S._engine()
    try:
        assert abs(float(eng.params.wheel_offset) - 0.2) < 1e-6
        batch = _lib.Batch(eng, 2)
        batch.set_dem(0, Z1)
        batch.set_wheel_log()
        batch.set_episode(0, S._as_given(t[0, 0]), seeds[0])
        batch.set_episode(1, S._as_given(t[0, 1]), seeds[1], dem=0)
        batch.set_tracking(max_steps=cap, runs_per_episode=2, keep_log=True, goal_tol=0.5, slope="wheels", metrics=True)
        cmds, dones = [], []
        for i in range(n):
            kw = dict(reset=S._dev(torch, [0, 1], torch.int32)) if i == reset_at else {}
            cmd, plan, done = batch.step_device(S._dev(torch, t[i]), z=S._dev(torch, z[i]), **kw)
            batch.engine.sync()
            cmds.append(cmd.cpu().numpy())
            dones.append(done.cpu().numpy())
        dones = np.array(dones)
        # episode 0: rows 0 .. 44 from ingests 1 .. 45, ended by the cap at ingest 45 and idle after
        assert (dones[:45, 0] == 0).all() and (dones[45:, 0] == 2).all()
        assert (dones[:, 1] == 0).all()
        assert list(batch.run_counts()) == [1, 1]
        scenes = [R.Scene(Z, hw, cm), R.Scene(Z1, hw, cm)]

        def rows_of(e, first, count):
            rows = np.array([[t[i, e, 0], t[i, e, 1], z[i, e], t[i, e, 2], t[i, e, 3], t[i, e, 4], cmds[i - 1][e, 0],
                              cmds[i - 1][e, 1]] for i in range(first, first + count)], F32).reshape(count, 8)
            wheels = np.array([_contacts(scenes[e], t[i, e, 0], t[i, e, 1], t[i, e, 2:5], off)
                               for i in range(first, first + count)], F32).reshape(count, 6)
            return rows, wheels

        # episode 0: the kept log, its wheel rows, the run's score and metrics
        rows0, wheels0 = rows_of(0, 1, cap)
        assert np.array_equal(_bits(batch.log(0)), _bits(rows0))
        got_w = batch.wheel_log(0)
        assert np.array_equal(_bits(got_w), _bits(wheels0)), (got_w[:3], wheels0[:3])
        assert np.array_equal(rows0[0, :3], rows0[21, :3]) and rows0[20, 2] == rows0[41, 2]
        run = batch.runs(0)
        assert run["status"][0] == 2 and run["rows"][0] == cap and run["status"][1] == 0
        after = batch.score(slope="wheels", metrics=True)
        assert _bits(run["cost"][0]) == _bits(after["cost"][0])
        assert np.array_equal(_bits(run["terms"][0]), _bits(after["terms"][0])), (run["terms"][0], after["terms"][0])
        assert run["collisions"][0] == after["collisions"][0]
        origin0 = V.origin_state(t[0, 0, 0], t[0, 0, 1], FAR[0], FAR[1])
        check_wheel_scores(dict((k, v[:1]) for k, v in after.items()), eng, [rows0], [wheels0], [origin0], "tracked")
        assert np.array_equal(_bits64(run["metrics"][0]), _bits64(path_metrics(rows0))), run["metrics"][0]
        assert np.array_equal(_bits64(after["metrics"][0]), _bits64(run["metrics"][0]))
        assert run["metrics"][0, 0] > 0 and not run["metrics"][1].any()
        body = batch.score()
        assert body["terms"][0, 1] != after["terms"][0, 1]
        # episode 1 (a DEM slot): the abandoned run of 29 rows, then the run in progress
        rows1, wheels1 = rows_of(1, 1, reset_at - 1)
        run1 = batch.runs(1)
        assert run1["status"][0] == 3 and run1["rows"][0] == reset_at - 1 and run1["status"][1] == 0
        origin1 = V.origin_state(t[0, 1, 0], t[0, 1, 1], FAR[0], FAR[1])
        want = score_wheels(eng, rows1, wheels1, origin1)
        assert _bits(run1["cost"][0]) == _bits(F32(want["cost"])), (run1["cost"][0], want["cost"])
        assert np.array_equal(_bits(run1["terms"][0]), _bits(np.asarray(want["terms"], F32)))
        assert np.array_equal(_bits64(run1["metrics"][0]), _bits64(path_metrics(rows1))), run1["metrics"][0]
        assert not run1["metrics"][0].any()      # its one segment is the repeated pose's: length 0, no angle
        rows1b, wheels1b = rows_of(1, reset_at + 1, n - 1 - reset_at)
        assert np.array_equal(_bits(batch.log(1)), _bits(rows1b))
        assert np.array_equal(_bits(batch.wheel_log(1)), _bits(wheels1b))
        assert not np.array_equal(wheels1b[:, 2], rows_of(0, reset_at + 1, n - 1 - reset_at)[1][:, 2])    # the slot acts
        batch.close()
    finally:
        eng.close()


# ---- 5. off means untouched; the refusals ----
def test_unchanged_when_off():
    S._gpu()
    from helpers import c3_scene
    from mppi_amd import _lib
    Z, hw, cm = c3_scene()
    eps = [(s, g, seed) for s, g, seed, _ in B.MAIN[:3]]
    refs = [B.engine_loop(K, H, Z, hw, cm, B.start_state(s, g), seed, 8) for s, g, seed in eps]
    eng = V.make_engine(K, H)
    try:
        for toggled in (False, True):
            batch = _lib.Batch(eng, len(eps))
            if toggled:      # on and off again before anything is set
                batch.set_wheel_log(True)
                batch.set_wheel_log(False)
                batch._score_options("wheels", True)
                batch._score_options("body", False)
            _set(batch, eps)
            batch.run(8, "3d", _policy())
            for e in range(len(eps)):
                V.same(V.collect(batch, e), refs[e], f"episode {e}, toggled {toggled}")
            with pytest.raises(RuntimeError, match="mppi_batch_set_wheel_log"):
                batch.score(slope="wheels")
            with pytest.raises(RuntimeError, match="wheel log"):
                batch.wheel_log(0, 0, 1)
            V.check_scores(batch.score(), eng, [batch.log(e) for e in range(len(eps))], _origins(eps), "body")
            batch.close()
    finally:
        eng.close()


def test_which_tables_exist_when():
    """The combinations the getters can see (csrc/mppi_batch_wheels.h has them all on the CPU): the wheel log
    on without a log, the score options on for a plain list, and the log's wheel array dropped when
    tracking lays the log out again without the option."""
    torch = S._gpu()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 2)
        lib, h = batch.lib, batch.h
        tasks = [_lib.make_task(V.mppi_state(B.start_state(STARTS[0], FAR)), s, 4) for s in (1, 2)]

        def run_list():
            done = 0
            while done < len(tasks):
                done, _ = batch.run_tasks(100, "3d", _policy())

        # the wheel log on, a list that keeps no log: no wheel log either; the online wheel chain still runs
        batch.set_wheel_log()
        batch.set_tasks(tasks, scored=True, keep_log=False, slope="wheels")
        run_list()
        log_free = batch.task_scores()
        with pytest.raises(RuntimeError, match="keeps no wheel log"):
            batch.task_wheel_log(0, 0, 1)
        with pytest.raises(RuntimeError, match="keeps no log"):
            batch.score_tasks(slope="wheels")
        # the score options on, a plain list: it takes neither, and is the plain list's run
        batch._score_options("wheels", True)
        batch.set_tasks(tasks)
        run_list()
        assert lib.mppi_batch_get_task_metrics(h, 0, 1, None) == MPPI_ESTATE
        assert batch.task_wheel_log(0).shape == (4, 6)        # (the wheel log is still on, and the list logs)
        after = batch.score_tasks(slope="wheels")
        assert np.array_equal(_bits(after["terms"]), _bits(log_free["terms"]))
        logs = [batch.task_log(i) for i in range(2)]
        batch.set_wheel_log(False)
        batch._score_options("body", False)
        batch.set_tasks(tasks)
        run_list()
        assert all(np.array_equal(_bits(batch.task_log(i)), _bits(logs[i])) for i in range(2))
        with pytest.raises(RuntimeError, match="keeps no wheel log"):
            batch.task_wheel_log(0, 0, 1)
        # a run with the wheel log; log-free tracking leaves the run's log and wheel rows readable
        batch.set_wheel_log()
        _set(batch, [(STARTS[0], FAR, 5), (STARTS[1], FAR, 6)])
        batch.run(3, "3d", _policy())
        rows = batch.wheel_log(0)
        assert rows.shape == (3, 6)
        batch.set_tracking(max_steps=4, keep_log=False)
        assert np.array_equal(_bits(batch.wheel_log(0)), _bits(rows))
        t = S._table(3, 2, 9)
        for i in range(3):
            batch.step_device(S._dev(torch, t[i]))
        batch.engine.sync()
        assert np.array_equal(_bits(batch.wheel_log(0)), _bits(rows))     # a log-free tracked step writes no wheel row
        # the option off, tracking lays the log out again: the wheel array goes
        batch.clear_tracking()
        batch.set_wheel_log(False)
        batch.set_tracking(max_steps=4, keep_log=True)
        with pytest.raises(RuntimeError, match="no wheel log"):
            batch.wheel_log(0, 0, 0)
        with pytest.raises(RuntimeError, match="mppi_batch_set_wheel_log"):
            batch.score(slope="wheels")
        batch.close()
    finally:
        eng.close()


def test_dm_atan2_on_the_device():
    """The device's dm_atan2 is the numpy restatement's, bit for bit, on the CPU test's grid; its distance
    from the device library's own atan2 and from numpy.arctan2 is printed and bounded as on the CPU
    (tests/test_path_metrics_cpu.py: the measured maximum of 6 ulp, plus 1)."""
    S._gpu()
    from mppi_amd.batch import dm_atan2
    from test_path_metrics_cpu import ATAN2_ULP, _grid, _ulps
    v = _grid()
    y, x = np.meshgrid(v, v)
    eng = V.make_engine(K, H)
    try:
        dm, dev = eng.detmath_atan2(y, x)
    finally:
        eng.close()
    want = dm_atan2(y, x)
    assert np.array_equal(_bits64(dm), _bits64(want)), int((_bits64(dm) != _bits64(want)).sum())
    ref = np.arctan2(y, x)
    nz = (ref != 0) & (dev != 0)
    assert np.all(dm[ref == 0] == 0)
    u_dev, u_np = _ulps(dm[nz], dev[nz]), _ulps(dm[nz], ref[nz])
    print("dm_atan2 on the device:", y.size, "points; max ulp from the device's atan2", u_dev.max(), ", from numpy's",
          u_np.max(), "; the device's atan2 from numpy's", _ulps(dev[nz], ref[nz]).max())
    assert u_np.max() <= ATAN2_ULP
    # from the device's own atan2: dm_atan2 is within 6 ulp of numpy's (measured on the CPU, and the bits are
    # the same here), numpy's (glibc) is within 1 ulp of the true value and the device library documents
    # 2 ulp for its float64 atan2: 6 + 1 + 2
    assert u_dev.max() <= 9


def test_refusals():
    torch = S._gpu()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 2)
        lib, h = batch.lib, batch.h
        fp = C.POINTER(C.c_float)
        row = np.zeros(6, F32)
        assert lib.mppi_batch_set_score_options(h, 7, 0) == MPPI_EINVAL
        assert lib.mppi_batch_score_ex(h, None, None, 7, C.byref(_lib.MppiPathScores()), None, None) == MPPI_EINVAL
        # a list without the wheel log: no wheel form after the run
        tasks = [_lib.make_task(V.mppi_state(B.start_state(STARTS[0], FAR)), s, 30) for s in (1, 2, 3)]
        batch.set_tasks(tasks)
        with pytest.raises(RuntimeError, match="mppi_batch_set_wheel_log"):
            batch.score_tasks(slope="wheels")
        assert lib.mppi_batch_get_task_metrics(h, 0, 1, None) == MPPI_ESTATE
        # options during a campaign
        batch.set_wheel_log()
        batch.set_tasks(tasks, scored=dict(slope="wheels", metrics=True))
        batch.run_tasks(2, "3d", _policy())
        assert lib.mppi_batch_set_wheel_log(h, 0) == MPPI_ESTATE and b"campaign" in lib.mppi_last_error()
        assert lib.mppi_batch_set_score_options(h, 1, 0) == MPPI_ESTATE and b"campaign" in lib.mppi_last_error()
        done = 0
        while done < 3:
            done, _ = batch.run_tasks(1000, "3d", _policy())
        # out-of-range getters
        assert lib.mppi_batch_get_task_wheel_log(h, 0, 0, 31, row.ctypes.data_as(fp)) == MPPI_EINVAL
        assert lib.mppi_batch_get_task_wheel_log(h, 3, 0, 1, row.ctypes.data_as(fp)) == MPPI_EINVAL
        assert lib.mppi_batch_get_task_wheel_log(h, 0, -1, 1, row.ctypes.data_as(fp)) == MPPI_EINVAL
        assert lib.mppi_batch_get_task_metrics(h, 2, 2, None) == MPPI_EINVAL
        assert batch.task_wheel_log(2).shape == (30, 6) and batch.task_scores()["metrics"].shape == (3, 4)
        assert lib.mppi_batch_get_wheel_log(h, 2, 0, 0, None) == MPPI_EINVAL
        # under tracking
        t = S._table(1, 2, 5)
        batch.set_episode(0, S._as_given(t[0, 0]), 1)
        batch.set_tracking(max_steps=4, metrics=True)
        assert lib.mppi_batch_set_wheel_log(h, 0) == MPPI_ESTATE and b"tracking" in lib.mppi_last_error()
        assert lib.mppi_batch_set_score_options(h, 0, 0) == MPPI_ESTATE and b"tracking" in lib.mppi_last_error()
        assert lib.mppi_batch_get_run_metrics(h, 0, 0, 2, None) == MPPI_EINVAL
        assert lib.mppi_batch_get_wheel_log(h, 0, 0, 1, row.ctypes.data_as(fp)) == MPPI_EINVAL     # no row yet
        batch.set_tracking(max_steps=4)
        assert lib.mppi_batch_get_run_metrics(h, 0, 0, 1, None) == MPPI_ESTATE
        batch.close()
    finally:
        eng.close()
