"""GPU: a scored task list (mppi_batch_set_tasks_scored / _get_task_scores): the lane
that runs a task scores it row by row, with or without a log.

Contract, per ended task: cost, terms, collisions and rows are bit for bit what
mppi_batch_score_tasks(b, yardstick, NULL, ...) returns for the logged run of the same list, and
`length` is compute_length of evaluate_trajectory.py:43-53 in float64 (mppi_amd.batch.path_length, the
numpy restatement, on the task's log).  A list that keeps no log gives the same score rows and results.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V

pytestmark = pytest.mark.gpu

MPPI_EINVAL, MPPI_ESTATE = -1, -3
K, H = 256, 20
FAR = (65.0, 10.0)
NEAR0, NEAR2, INSIDE = B.MAIN[0][:3], B.MAIN[2][:3], B.MAIN[3][:3]     # (start, goal, seed)
HORIZON = 0.045 * 2.0 * H         # make_params' default: dt * v_max_linear * H


def far(seed):
    return (B.START, FAR, seed)


# (start, goal, seed), cap.  Far-goal tasks run to their cap: path lengths 1-6, 11-13 and 26 (the
# scorer's chunk is 12 waypoints; odd and even lengths end the slope chain differently; 6 and 11
# are one past a sampled row of `length`).  Near-goal tasks take the other path-follow branch, two of
# them to the goal before their cap, three cut short at 1, 2 and 3 rows.  Zero-step tasks first, in
# the middle and last.
MAIN = [(INSIDE, 5), (far(1), 1), (far(2), 2), (NEAR0, 40), (far(3), 3), (far(4), 4), (far(5), 5), (INSIDE, 1),
        (far(6), 6), (NEAR0, 1), (far(11), 11), (far(12), 12), (NEAR2, 40), (far(13), 13), (NEAR0, 2), (far(26), 26),
        (NEAR2, 3), (INSIDE, 3)]
LANES = (1, 3, 16)                # 16 > the tasks that take steps at once


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _policy(check_every=0):
    from mppi_amd import _lib
    return _lib.make_policy(check_every=check_every, **B.RUN)


def _state(start, goal):
    return V.mppi_state(B.start_state(start, goal))


def _tasks(main, **kw):
    from mppi_amd import _lib
    return [_lib.make_task(_state(start, goal), seed, cap, **kw) for (start, goal, seed), cap in main]


def _final(s):
    return np.array([s.x, s.y, s.heading[0], s.heading[1], s.heading[2], s.left_wheel_speed, s.right_wheel_speed,
                     s.goal_x, s.goal_y, s.std_dev_u1, s.std_dev_u2], np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(batch, n, budget=100000, check_every=0, proj="3d"):
    done, total, calls = 0, 0, 0
    while done < n:
        done, steps = batch.run_tasks(budget, proj, _policy(check_every))
        assert steps <= budget
        total += steps
        calls += 1
        assert calls < 1000
    return total


def _results(batch, n):
    out = []
    for i in range(n):
        info = batch.task(i)
        out.append(dict(final=_final(info["state"]), steps=info["steps"], reached=info["reached"],
                        started=info["started"]))
    return out


def _same_scores(got, want, tag, keys=("cost", "terms", "collisions", "rows", "length")):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        if k == "length":
            assert np.array_equal(_bits64(g), _bits64(w)), (tag, k, g, w)
        elif g.dtype == np.float32:
            assert np.array_equal(_bits(g), _bits(w)), (tag, k, g, w)
        else:
            assert np.array_equal(g, w), (tag, k, g, w)


def _same_results(got, want, tag):
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g["steps"], g["reached"], g["started"]) == (w["steps"], w["reached"], w["started"]), (tag, i, g, w)
        assert np.array_equal(_bits(g["final"]), _bits(w["final"])), (tag, i)


def _lengths(logs):
    from mppi_amd.batch import path_length
    return np.array([path_length(r) for r in logs], np.float64)


@functools.lru_cache(maxsize=None)
def _main_scored(lanes, keep_log=True, budget=100000, check_every=0):
    """MAIN set scored with the default yardstick and run to its end: the online scores, the results
    and, with a log, the logs and the log scorer's answer of the same batch."""
    _gpu()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, lanes)
        batch.set_tasks(_tasks(MAIN), scored=True, keep_log=keep_log)
        _run(batch, len(MAIN), budget, check_every)
        out = dict(online=batch.task_scores(), results=_results(batch, len(MAIN)))
        if keep_log:
            out["logs"] = [batch.task_log(i) for i in range(len(MAIN))]
            out["scorer"] = batch.score_tasks()
        batch.close()
    finally:
        eng.close()
    return out


# ---- 1. bitwise against the log scorer ----
def test_main_list_covers_the_cases():
    """From the results themselves: every path length of the issue, both path-follow branches, a goal
    reached before the cap, and zero-step tasks."""
    r = _main_scored(3)
    steps = [x["steps"] for x in r["results"]]
    assert {0, 1, 2, 3, 4, 5, 6, 11, 12, 13} <= set(steps), steps
    assert max(steps) >= 26
    dist = [float(np.hypot(g[0] - s[0], g[1] - s[1])) for (s, g, _), _ in MAIN]
    ran = [i for i, n in enumerate(steps) if n > 0]
    assert any(dist[i] > HORIZON for i in ran) and any(dist[i] < HORIZON for i in ran)
    # the near branch with 1, 2, 3 and more rows: its held-back term at every length
    assert {1, 2, 3} <= {steps[i] for i in ran if dist[i] < HORIZON}
    assert any(steps[i] > 3 for i in ran if dist[i] < HORIZON)
    early = [i for i in ran if r["results"][i]["reached"] and steps[i] < MAIN[i][1]]
    assert early, steps
    assert all(x["started"] == 2 for x in r["results"])
    # the scores are not trivially equal: every task that ran has a cost, and the lengths differ
    assert all(r["online"]["cost"][i] != 0 for i in ran)
    assert len({float(v) for v in r["online"]["length"]}) > 4


@pytest.mark.parametrize("lanes", LANES)
def test_online_scores_are_the_log_scorers(lanes):
    r = _main_scored(lanes)
    got = r["online"]
    N = len(MAIN)
    assert got["cost"].shape == (N,) and got["terms"].shape == (N, 4) and got["length"].dtype == np.float64
    _same_scores(got, r["scorer"], f"{lanes} lanes", keys=("cost", "terms", "collisions", "rows"))
    assert list(got["rows"]) == [x["steps"] for x in r["results"]] == [len(l) for l in r["logs"]]
    want = _lengths(r["logs"])
    assert np.array_equal(_bits64(got["length"]), _bits64(want)), (got["length"], want)
    for i, x in enumerate(r["results"]):
        if x["steps"] == 0:         # a row of zeros
            assert got["cost"][i] == 0 and not got["terms"][i].any() and got["collisions"][i] == 0
            assert got["length"][i] == 0
        if x["steps"] > 5:
            assert got["length"][i] > 0
    # the lane shows in no result
    _same_scores(got, _main_scored(LANES[0])["online"], f"{lanes} lanes vs {LANES[0]}")
    _same_results(r["results"], _main_scored(LANES[0])["results"], f"{lanes} lanes vs {LANES[0]}")


def test_partial_ranges():
    """first / count address the rows; an empty range and a range outside the list."""
    _gpu()
    from mppi_amd import _lib
    want = _main_scored(3)["online"]
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 3)
        batch.set_tasks(_tasks(MAIN), scored=True)
        _run(batch, len(MAIN))
        part = batch.task_scores(5, 7)
        _same_scores(part, {k: v[5:12] for k, v in want.items()}, "rows 5..11")
        assert batch.task_scores(4, 0)["cost"].shape == (0,)
        length = (C.c_double * 2)()
        assert batch.lib.mppi_batch_get_task_scores(batch.h, 10, 2, None, None, length) == 0     # any output may be NULL
        assert np.array_equal(_bits64(np.array(length[:])), _bits64(want["length"][10:12]))
        rc = batch.lib.mppi_batch_get_task_scores(batch.h, len(MAIN) - 1, 2, None, None, length)
        assert rc == MPPI_EINVAL and b"outside the list" in batch.lib.mppi_last_error()
        batch.close()
    finally:
        eng.close()


# ---- 2. against the CPU oracle ----
@pytest.mark.parametrize("i", [11, 15])
def test_online_terms_are_the_oracles(i):
    r = _main_scored(3)
    (start, goal, _), cap = MAIN[i]
    assert cap in (12, 26) and len(r["logs"][i]) == cap
    terms, col = V.oracle_terms(r["logs"][i], start, goal, HORIZON)
    assert np.array_equal(_bits(r["online"]["terms"][i]), _bits(terms)), (i, r["online"]["terms"][i], terms)
    assert r["online"]["collisions"][i] == col


# ---- 3. a yardstick off the defaults ----
YARD = dict(w_path=3.0, w_slope=5.0, w_speed=7.0, w_obstacle=11.0, collision_threshold=0.5, collision_penalty=1000.0)
FULL_SLOT = 7


def test_yardstick_off_the_defaults():
    """Weights (3, 5, 7, 11), threshold 0.5, penalty 1000 and the context's w_orientation = 2: still
    bitwise the log scorer.  Tasks on a costmap slot filled with 1.0 (every row collides) and on the
    scene's own map, with and without a variant, one of them in the 2D projection."""
    _gpu()
    from helpers import c3_scene
    from mppi_amd import _lib
    from mppi_amd.batch import variant_dict
    _, _, cm = c3_scene()
    eng = V.make_engine(K, H)
    try:
        eng.set_critics("wheels", 2.0)
        batch = _lib.Batch(eng, 2)
        batch.set_costmap(FULL_SLOT, np.ones_like(cm))
        batch.set_variants([V.variant("proj2d"), variant_dict("3d", temperature=3.0)])
        mk = lambda t, cap, **kw: _lib.make_task(_state(t[0], t[1]), t[2], cap, **kw)
        tasks = [mk(far(50), 7, costmap=FULL_SLOT), mk(far(51), 6), mk(far(52), 5, variant=0),
                 mk(far(53), 9, variant=1, costmap=FULL_SLOT), mk(NEAR0, 40, variant=1), mk(INSIDE, 4, variant=0),
                 mk(NEAR2, 40, costmap=FULL_SLOT)]
        on_slot = [0, 3, 6]
        yard = _lib.make_variant(**YARD)
        batch.set_tasks(tasks, scored=yard)
        _run(batch, len(tasks))
        got = batch.task_scores()
        want = batch.score_tasks(yardstick=yard)
        default = batch.score_tasks()
        logs = [batch.task_log(i) for i in range(len(tasks))]
        batch.close()
    finally:
        eng.close()
    _same_scores(got, want, "yardstick", keys=("cost", "terms", "collisions", "rows"))
    assert np.array_equal(_bits64(got["length"]), _bits64(_lengths(logs)))
    assert list(got["rows"][:4]) == [7, 6, 5, 9] and got["rows"][5] == 0 and got["rows"][4] > 0
    for i in on_slot:
        assert got["collisions"][i] == got["rows"][i] > 0, i
    assert got["collisions"][1] < got["rows"][1]
    # the yardstick is read: the default one gives other costs for the same terms
    ran = [i for i in range(len(tasks)) if got["rows"][i] > 0]
    assert all(_bits(got["cost"][i]) != _bits(default["cost"][i]) for i in ran)


# ---- 4. log-free equals logged ----
@pytest.mark.parametrize("check_every", [1, 7])
def test_log_free_equals_logged(check_every):
    """keep_log = 0, the campaign split over calls of 3 batch steps: the same score rows and results,
    so the lanes' accumulators survive the host's looks; the log's readers answer MPPI_ESTATE."""
    want = _main_scored(3)
    got = _main_scored(3, False, 3, check_every)
    _same_scores(got["online"], want["online"], f"log-free, check_every {check_every}")
    _same_results(got["results"], want["results"], f"log-free, check_every {check_every}")


def test_log_free_refuses_the_logs_readers():
    _gpu()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 2)
        batch.set_tasks(_tasks([(far(1), 2), (INSIDE, 2)]), scored=True, keep_log=False)
        _run(batch, 2)
        assert batch.task(0)["steps"] == 2
        rows = np.zeros((2, 8), np.float32)
        sc = _lib.MppiPathScores()
        for rc in (batch.lib.mppi_batch_get_task_log(batch.h, 0, 0, 2, _lib._fp(rows)),
                   batch.lib.mppi_batch_get_task_log(batch.h, 1, 0, 0, None),
                   batch.lib.mppi_batch_score_tasks(batch.h, None, None, C.byref(sc), None)):
            assert rc == MPPI_ESTATE, rc
            assert b"keeps no log" in batch.lib.mppi_last_error()
        with pytest.raises(RuntimeError, match="keeps no log"):
            batch.task_log(0)
        with pytest.raises(RuntimeError, match="keeps no log"):
            batch.score_tasks()
        assert batch.task_scores()["rows"].tolist() == [2, 0]
        batch.close()
    finally:
        eng.close()


# ---- 5. beyond the arena ----
def test_beyond_the_arena():
    """Caps that sum above the book's 2^40-row limit: the logged list is refused, the scored log-free
    list runs and scores."""
    _gpu()
    from mppi_amd import _lib
    big = 2 ** 31 - 1
    main = [(INSIDE, big)] * 300 + [(far(4), 4)] + [(INSIDE, big)] * 220
    assert sum(cap for _, cap in main) > 2 ** 40
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 2)
        tasks = _tasks(main)
        arr = (_lib.MppiBatchTask * len(tasks))(*tasks)
        for rc in (batch.lib.mppi_batch_set_tasks(batch.h, len(tasks), arr),
                   batch.lib.mppi_batch_set_tasks_scored(batch.h, len(tasks), arr, None, 1)):
            assert rc == MPPI_EINVAL, rc
            assert b"too many log rows" in batch.lib.mppi_last_error()
        batch.set_tasks(tasks, scored=True, keep_log=False)
        steps = _run(batch, len(tasks))
        assert steps == 4
        got = batch.task_scores()
        res = _results(batch, len(tasks))
        assert [r["steps"] for r in res] == [0] * 300 + [4] + [0] * 220
        assert all(r["started"] == 2 for r in res)
        # the one real task scores as it does alone, with a log
        batch.set_tasks(_tasks([(far(4), 4)]), scored=True)
        _run(batch, 1)
        alone = batch.task_scores()
        _same_scores(alone, batch.score_tasks(), "alone", keys=("cost", "terms", "collisions", "rows"))
        batch.close()
    finally:
        eng.close()
    _same_scores({k: v[300:301] for k, v in got.items()}, alone, "task 300")
    assert got["rows"][300] == 4 and got["cost"][300] != 0
    rest = np.r_[0:300, 301:len(main)]
    assert not got["cost"][rest].any() and not got["terms"][rest].any() and not got["rows"][rest].any()
    assert not got["collisions"][rest].any() and not got["length"][rest].any()


# ---- 6. unended and unclaimed tasks; coexistence with plain lists ----
PLAIN = [(far(30), 3), (INSIDE, 2), (NEAR0, 40), (far(31), 5)]


def _plain_campaign(batch):
    batch.set_tasks(_tasks(PLAIN))
    _run(batch, len(PLAIN))
    return [dict(rows=batch.task_log(i), **r) for i, r in enumerate(_results(batch, len(PLAIN)))]


@functools.lru_cache(maxsize=None)
def _plain_alone():
    _gpu()
    from mppi_amd import _lib
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 2)
        out = _plain_campaign(batch)
        batch.close()
    finally:
        eng.close()
    return out


def test_unended_tasks_score_zero_and_plain_lists_are_undisturbed():
    _gpu()
    from mppi_amd import _lib
    alone = _plain_alone()
    assert [r["steps"] for r in alone][:2] == [3, 0] and alone[3]["steps"] == 5
    eng = V.make_engine(K, H)
    try:
        batch = _lib.Batch(eng, 2)

        def plain_again(tag):
            got = _plain_campaign(batch)
            _same_results(got, alone, tag)
            for i, (g, w) in enumerate(zip(got, alone)):
                assert np.array_equal(_bits(g["rows"]), _bits(w["rows"])), (tag, i)

        # before any list, and with a plain list: no scores
        for scored_yet in (False, True):
            if scored_yet:
                batch.set_tasks(_tasks(PLAIN))
            rc = batch.lib.mppi_batch_get_task_scores(batch.h, 0, 0, None, None, None)
            assert rc == MPPI_ESTATE and b"not set scored" in batch.lib.mppi_last_error()
        plain_again("before the scored campaign")
        # a scored list on two lanes, looked at after 2 and after 4 batch steps
        main = [(far(40), 2), (far(41), 6), (far(42), 3), (INSIDE, 2), (far(43), 4)]
        for keep_log in (True, False):
            batch.set_tasks(_tasks(main), scored=True, keep_log=keep_log)
            z = batch.task_scores()                                  # set, not started: all zeros
            assert not z["cost"].any() and not z["rows"].any() and not z["length"].any()
            done, steps = batch.run_tasks(2, "3d", _policy())
            assert (done, steps) == (1, 2)
            assert [batch.task(i)["started"] for i in range(5)] == [2, 1, 1, 0, 0]
            a = batch.task_scores()
            assert a["rows"].tolist() == [2, 0, 0, 0, 0] and a["cost"][0] != 0
            assert not a["cost"][1:].any() and not a["terms"][1:].any() and not a["collisions"][1:].any()
            assert not a["length"][1:].any()
            done, steps = batch.run_tasks(2, "3d", _policy())
            assert (done, steps) == (1, 2)
            b = batch.task_scores()
            assert b["rows"].tolist() == [2, 0, 0, 0, 0]             # task 2 has 2 of its 3 rows, task 1 4 of 6
            _run(batch, 5)
            c = batch.task_scores()
            assert c["rows"].tolist() == [2, 6, 3, 0, 4]
            _same_scores({k: v[:1] for k, v in c.items()}, {k: v[:1] for k, v in a.items()}, "task 0 stays")
            if keep_log:
                _same_scores(c, batch.score_tasks(), "split", keys=("cost", "terms", "collisions", "rows"))
                first = c
            else:
                _same_scores(c, first, "log-free split")
        # replaced by a plain list: the scores are gone, the plain campaign is what it was alone
        batch.set_tasks(_tasks(PLAIN))
        with pytest.raises(RuntimeError, match="not set scored"):
            batch.task_scores()
        plain_again("after the scored campaigns")
        batch.close()
    finally:
        eng.close()


# ---- MPPI_Controller.run_campaign ----
def test_run_campaign_log_free():
    """run_campaign(score=..., log=False): the scores of the logged campaign, no trails."""
    _gpu()
    from helpers import c3_scene
    from mppi_amd import controller
    from mppi_amd.batch import campaign_results, campaign_summary
    Z, hw, cm = c3_scene()
    cfg = controller._load_config(controller.DEFAULT_CONFIG)
    cfg = {**cfg, "controller": {**cfg["controller"], "number_of_trajectories": K, "number_of_iterations": H}}
    surface = controller.Surface.from_arrays(Z, cm, hw, radius_robot=0.3)
    robot = controller.Robot(B.START[0], B.START[1], [1.0, 0.0, 0.0], cfg)
    ctl = controller.MPPI_Controller(surface, robot, cfg, FAR[0], FAR[1], 0.0)
    ctl.std_dev_u1 = ctl.std_dev_u2 = 0.25
    main = [(far(60), 4), (NEAR0, 40), (far(61), 7), (INSIDE, 3)]
    args = dict(starts=[t[0] for t, _ in main], headings=[(1.0, 0.0, 0.0)] * 4, goals=[t[1] for t, _ in main],
                seeds=[t[2] for t, _ in main], lanes=2, max_loops=[cap for _, cap in main], score=True)
    try:
        res, scores = ctl.run_campaign(**args)
        res0, scores0 = ctl.run_campaign(log=False, **args)
        with pytest.raises(ValueError, match="log=False needs"):
            ctl.run_campaign(**{**args, "score": None, "log": False})
    finally:
        ctl.engine.close()
    _same_scores(scores0, scores, "run_campaign")
    assert [r["loops"] for r in res0] == [r["loops"] for r in res] == list(scores["rows"])
    assert [r["reached"] for r in res0] == [r["reached"] for r in res]
    assert all("lin_vel" not in r for r in res0)
    for r0, r in zip(res0[:3], res[:3]):
        assert _bits(r0["x"]) == _bits(r["x"][-1]) and _bits(r0["y"]) == _bits(r["y"][-1])
    table = campaign_summary(campaign_results(res0, scores0), by=["far", "near", "far", "near"])
    assert table["far"]["count"] == 2 and table["far"]["reached"] == 0 and table["near"]["reached"] == 2
    assert table["far"]["mean"]["length"] == float(np.mean(scores["length"][[0, 2]]))
