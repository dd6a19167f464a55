"""GPU: batched closed-loop episodes (include/mppi.h mppi_batch_*).

Every episode of a batch is compared bit for bit (log rows, final state, final nominal sequence,
step counts, `reached`) with the closed loops of tests/batch_refs.py on the C1-C4 scene:
  reference A  the loop over oracle.mppi_ref.mppi_step (CPU)
  reference B  the loop over a fresh Engine(seed=seed_e).step, stepped from the host
both with the advance rule written out in the test helpers and the raw row-0 heading passed on.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import batch_refs as B

pytestmark = pytest.mark.gpu

FAR = (65.0, 10.0)


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _engine(K, H, **options):
    from helpers import c3_scene
    from mppi_amd import _lib
    Z, hw, cm = c3_scene()
    eng = _lib.Engine(_lib.make_params(K, H), 0)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    return eng


def _mppi_state(st):
    from mppi_amd import _lib
    s = _lib.MppiState()
    s.x, s.y = float(st["x"]), float(st["y"])
    for i in range(3):
        s.heading[i] = float(np.float32(st["heading"][i]))   # used as given
    s.left_wheel_speed, s.right_wheel_speed = float(st["wl"]), float(st["wr"])
    s.goal_x, s.goal_y = float(st["gx"]), float(st["gy"])
    s.std_dev_u1, s.std_dev_u2 = float(st["s1"]), float(st["s2"])
    return s


def _collect(batch, e, rows=None):
    info = batch.episode(e)
    s = info["state"]
    final = np.array([s.x, s.y, s.heading[0], s.heading[1], s.heading[2], s.left_wheel_speed, s.right_wheel_speed,
                      s.goal_x, s.goal_y, s.std_dev_u1, s.std_dev_u2], np.float32)
    return dict(rows=batch.log(e) if rows is None else rows, final=final, u1=info["u1"], u2=info["u2"],
                steps=info["steps_last_run"], total=info["steps_total"], reached=info["reached"])


def _run_batch(K, H, episodes, runs, proj="3d", pol=B.RUN, check_every=0):
    """episodes: [(state dict, seed)]; runs: step caps of successive mppi_batch_run calls.  Returns
    per episode the result after the last run, its log rows those of all runs concatenated."""
    _gpu()
    from mppi_amd import _lib
    eng = _engine(K, H)
    try:
        batch = _lib.Batch(eng, len(episodes))
        for e, (st, seed) in enumerate(episodes):
            batch.set_episode(e, _mppi_state(st), seed)
        policy = _lib.make_policy(check_every=check_every, **pol)
        logs = [[] for _ in episodes]
        totals = [0] * len(episodes)
        for n in runs:
            batch.run(n, proj, policy)
            for e in range(len(episodes)):
                logs[e].append(batch.log(e))
                totals[e] += batch.episode(e)["steps_last_run"]
        out = []
        for e in range(len(episodes)):
            r = _collect(batch, e, np.concatenate(logs[e]))
            assert r["total"] == totals[e], (e, r["total"], totals[e])
            r["steps"] = totals[e]
            out.append(r)
        ms = batch.last_ms()
        assert ms > 0.0
        batch.close()
    finally:
        eng.close()
    return out


def _same(got, ref, tag):
    assert got["steps"] == ref["steps"], (tag, got["steps"], ref["steps"])
    assert got["reached"] == ref["reached"], tag
    np.testing.assert_array_equal(got["rows"], ref["rows"], err_msg=f"log rows {tag}")
    np.testing.assert_array_equal(got["final"], ref["final"], err_msg=f"final state {tag}")
    np.testing.assert_array_equal(got["u1"], ref["u1"], err_msg=f"nominal u1 {tag}")
    np.testing.assert_array_equal(got["u2"], ref["u2"], err_msg=f"nominal u2 {tag}")


def _ref_b(K, H, st, seed, n, proj="3d", pol=B.RUN):
    from helpers import c3_scene
    Z, hw, cm = c3_scene()
    return B.engine_loop(K, H, Z, hw, cm, dict(st), seed, n, proj, pol)


def _ref_a(K, H, st, seed, n, proj="3d", pol=B.RUN):
    from helpers import c3_scene, oracle_scene
    return B.oracle_loop(K, H, oracle_scene(*c3_scene()), dict(st), seed, n, proj, pol)


@pytest.mark.parametrize("which", ["large_angle", "nonsquare"])
def test_off_default_parameters_and_geometry(which):
    """2 episodes x 3 steps on a context created with test_gpu_param_space's large-angle parameters
    (the batch fills the rollout's small_angle itself), and on its 120 x 200 DEM with x_min != -y_min,
    from the map's lower left corner: equal to the engine-stepped loop and to the oracle's."""
    _gpu()
    import helpers as hp
    import test_gpu_param_space as PS
    from mppi_amd import _lib
    K, H, n = 256, 16, 3
    if which == "large_angle":
        c, starts = PS.LARGE_ANGLE, [((-12.0, -3.0), (1.0, 0.0, 0.0)), ((3.0, 4.0), (0.0, -1.0, 0.0))]
        assert not PS._small_angle_rule(c)
    else:
        c, starts = PS.GEOMETRY["nonsquare_corner"], [((-29.9, -19.5), (-1.0, 0.0, 0.0)), ((-29.5, -19.9), (0.0, -1.0, 0.0))]
    sc, params = PS._scene(c.scene), dict(c.params)

    def make_engine(seed):
        eng = _lib.Engine(_lib.make_params(K, H, seed=seed, **params), 0)
        hp.bind_scene(eng, sc)
        return eng

    episodes = []
    for e, (start, heading) in enumerate(starts):
        st = B.start_state(start, PS.GOAL, heading, s1=0.8, s2=0.8)
        st["wl"], st["wr"] = np.float32(0.6), np.float32(0.8)
        episodes.append((st, 11 + e))
    eng = make_engine(42)
    try:
        batch = _lib.Batch(eng, len(episodes))
        for e, (st, seed) in enumerate(episodes):
            batch.set_episode(e, _mppi_state(st), seed)
        batch.run(n, "3d", _lib.make_policy(**B.RUN))
        got = [_collect(batch, e) for e in range(len(episodes))]
        batch.close()
    finally:
        eng.close()
    p = dataclasses.replace(c.oracle_params(), K=K, H=H)
    for e, (st, seed) in enumerate(episodes):
        assert got[e]["steps"] == n
        _same(got[e], B.engine_loop(K, H, None, None, None, dict(st), seed, n, make_engine=make_engine),
              f"{which} episode {e} vs B")
        _same(got[e], B.oracle_loop(K, H, sc, dict(st), seed, n, params=p), f"{which} episode {e} vs A")


def _main_episodes():
    return [(B.start_state(start, goal), seed) for start, goal, seed, _ in B.MAIN]


@functools.lru_cache(maxsize=None)
def _main_batch(check_every=0):
    return _run_batch(256, 20, _main_episodes(), (40,), check_every=check_every)


def test_main_case_k256():
    """H = 20, run() policy, 40 steps, one batch of E = 5 at K = 256: three episodes that reach their
    goal after different numbers of steps, one that starts inside the tolerance, one that runs to the
    cap.  (Episode 1's K = 300 runs in test_main_case_k300; here its slot runs at K = 256.)"""
    got = _main_batch()
    for e, (st, seed) in enumerate(_main_episodes()):
        b = _ref_b(256, 20, st, seed, 40)
        a = B.oracle_main(e) if B.MAIN[e][3] == 256 else _ref_a(256, 20, st, seed, 40)
        print(f"episode {e}: batch {got[e]['steps']} steps, A {a['steps']}, B {b['steps']}")
        if e < 4:   # the references stop by the goal test: not every episode runs into the cap
            assert a["steps"] < 40 and b["steps"] < 40 and a["reached"] and b["reached"], e
        _same(got[e], b, f"episode {e} vs B")
        _same(got[e], a, f"episode {e} vs A")
    assert got[3]["steps"] == 0 and got[3]["reached"]      # starts inside the tolerance: no step
    assert got[4]["steps"] == 40 and not got[4]["reached"]
    assert len({got[e]["steps"] for e in range(5)}) >= 3   # the episodes stop at different steps


def test_main_case_k300():
    """Episode 1 of the main case (K = 300: a ragged second leaf) with a far-goal episode."""
    start, goal, seed, K = B.MAIN[1]
    eps = [(B.start_state(start, goal), seed), (B.start_state(B.START, FAR), 1)]
    got = _run_batch(K, 20, eps, (40,))
    a1 = B.oracle_main(1)
    assert a1["steps"] < 40 and a1["reached"]
    _same(got[0], a1, "episode 1 vs A")
    for e, (st, sd) in enumerate(eps):
        b = _ref_b(K, 20, st, sd, 40)
        assert e == 1 or b["steps"] < 40
        _same(got[e], b, f"K=300 episode {e} vs B")
    assert got[1]["steps"] == 40 and not got[1]["reached"]


def test_k1280_padded_tree():
    """5 leaf records: the finish's tree is padded to 8."""
    eps = [(B.start_state(B.START, FAR), 11), (B.start_state((10.0, 12.0), (40.0, -20.0), (0.0, 1.0, 0.0)), 12)]
    got = _run_batch(1280, 20, eps, (4,))
    for e, (st, sd) in enumerate(eps):
        _same(got[e], _ref_b(1280, 20, st, sd, 4), f"K=1280 episode {e} vs B")
        _same(got[e], _ref_a(1280, 20, st, sd, 4), f"K=1280 episode {e} vs A")
        assert got[e]["steps"] == 4


def test_odd_horizon():
    """H = 21: the half Philox block at the row end and the 4-float padding of the nominal sequence."""
    eps = [(B.start_state(B.START, FAR), 5), (B.start_state((10.0, 12.0), FAR), 6)]
    got = _run_batch(256, 21, eps, (3,))
    for e, (st, sd) in enumerate(eps):
        _same(got[e], _ref_b(256, 21, st, sd, 3), f"H=21 episode {e} vs B")
        assert got[e]["steps"] == 3


def test_2d_projection_isaac_policy():
    h = (0.6, 0.8, 0.0)
    eps = [(B.start_state(B.START, FAR, h), 21), (B.start_state((10.0, 12.0), FAR, h), 22)]
    got = _run_batch(256, 20, eps, (12,), proj="2d", pol=B.ISAAC)
    for e, (st, sd) in enumerate(eps):
        _same(got[e], _ref_b(256, 20, st, sd, 12, "2d", B.ISAAC), f"2d episode {e} vs B")
        _same(got[e], _ref_a(256, 20, st, sd, 12, "2d", B.ISAAC), f"2d episode {e} vs A")
        assert got[e]["steps"] == 12
    # the policy is in use: the sigmas sit at its base or above, not at run()'s 0.4
    assert got[0]["final"][9] == np.float32(0.25) or got[0]["final"][10] > np.float32(0.25)
    assert got[0]["final"][9] < np.float32(0.4)


@pytest.mark.parametrize("check_every", [1, 7])
def test_check_every_does_not_change_results(check_every):
    ref = _main_batch()
    got = _run_batch(256, 20, _main_episodes(), (40,), check_every=check_every)
    for e in range(5):
        _same(got[e], ref[e], f"check_every={check_every} episode {e}")


def test_split_runs_continue():
    """run(3) then run(3) = run(6): state, nominal and the concatenated log; the step index keeps counting."""
    eps = _main_episodes()
    whole = _run_batch(256, 20, eps, (6,))
    split = _run_batch(256, 20, eps, (3, 3))
    for e in range(5):
        _same(split[e], whole[e], f"split episode {e}")
    assert whole[4]["steps"] == 6 and whole[3]["steps"] == 0


def test_context_is_undisturbed():
    """Three Engine.step calls give the same bits with a batch run between steps 1 and 2 as without;
    the resident server was stopped for the batch, not failed."""
    _gpu()
    from mppi_amd import _lib
    names = ("u1_opt", "u2_opt", "lin_vel", "ang_vel", "traj_sim", "heading_sim")

    def steps(with_batch):
        eng = _engine(256, 20, resident=2, resident_idle_us=100000)
        try:
            eng.set_state(_lib.make_state(B.START[0], B.START[1], goal_x=FAR[0], goal_y=FAR[1]))
            outs = []
            for i in range(3):
                if with_batch and i == 2:
                    batch = _lib.Batch(eng, 2)
                    batch.set_episode(0, _mppi_state(B.start_state((10.0, 12.0), FAR)), 3)
                    batch.set_episode(1, _mppi_state(B.start_state(B.START, (-59.3, -4.9))), 7)
                    batch.run(5)
                    assert batch.episode(0)["steps_last_run"] == 5
                    batch.close()
                o = eng.step("3d", i)
                outs.append({k: o[k].copy() for k in names})
            return outs, eng.costs().copy(), eng.get_nominal(), eng.launch_info()
        finally:
            eng.close()

    (o0, c0, n0, i0), (o1, c1, n1, i1) = steps(False), steps(True)
    for i in range(3):
        for k in names:
            np.testing.assert_array_equal(o1[i][k], o0[i][k], err_msg=f"step {i} {k}")
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(n1[0], n0[0])
    np.testing.assert_array_equal(n1[1], n0[1])
    for info in (i0, i1):
        assert info["server_steps"] == 3 and info["server_failed_steps"] == 0 and info["server_fallbacks"] == 0, info
    assert i1["server_launches"] == i0["server_launches"] + 1, (i0, i1)   # stopped for the batch, launched again


def test_arguments_and_state_checks():
    _gpu()
    from mppi_amd import _lib
    lib = _lib.load_library()
    eng = _lib.Engine(_lib.make_params(256, 20), 0)
    big = _lib.Engine(_lib.make_params(4097, 20), 0)    # 17 leaf records
    try:
        h = ctypes.c_void_p()
        assert lib.mppi_batch_create(big.ctx, 2, ctypes.byref(h)) == -1 and not h.value
        assert lib.mppi_batch_create(eng.ctx, 4097, ctypes.byref(h)) == -1 and not h.value
        batch = _lib.Batch(eng, 3)
        st = _mppi_state(B.start_state(B.START, FAR))
        pol = _lib.make_policy()
        for e in (-1, 3):
            assert lib.mppi_batch_set_episode(batch.h, e, ctypes.byref(st), 1) == -1
            assert lib.mppi_batch_get_episode(batch.h, e, None, None, None, None, None, None) == -1
            assert lib.mppi_batch_get_log(batch.h, e, 0, 0, None) == -1
        assert lib.mppi_batch_set_episode(batch.h, 0, None, 1) == -1
        assert lib.mppi_batch_run(batch.h, 3, 1, None) == -1
        assert lib.mppi_batch_run(batch.h, 4, 1, ctypes.byref(pol)) == -1      # proj
        assert lib.mppi_batch_run(batch.h, 3, -1, ctypes.byref(pol)) == -1
        batch.set_episode(1, st, 9)
        assert lib.mppi_batch_run(batch.h, 3, 2, ctypes.byref(pol)) == -3       # MPPI_ESTATE: no DEM, no costmap
        from helpers import c3_scene
        Z, hw, cm = c3_scene()
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        batch.run(2)
        # an episode never set does not run
        assert [batch.episode(e)["steps_last_run"] for e in range(3)] == [0, 2, 0]
        assert not batch.episode(0)["reached"] and batch.episode(1)["steps_total"] == 2
        rows = np.zeros((3, 8), np.float32)
        fp = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        assert lib.mppi_batch_get_log(batch.h, 1, 0, 3, fp) == -1               # beyond steps_last_run
        assert lib.mppi_batch_get_log(batch.h, 1, 1, 1, fp) == 0
        np.testing.assert_array_equal(rows[0], batch.log(1)[1])
        batch.close()
    finally:
        eng.close()
        big.close()


def test_run_batch_returns_the_trails():
    """MPPI_Controller.run_batch on two episodes: the lists Robot accumulates are the log's columns."""
    _gpu()
    from helpers import c3_scene
    from mppi_amd import controller
    Z, hw, cm = c3_scene()
    cfg = controller._load_config(controller.DEFAULT_CONFIG)
    cfg = {**cfg, "controller": {**cfg["controller"], "number_of_trajectories": 256, "number_of_iterations": 20},
           "engine": {**(cfg.get("engine") or {}), "seed": 7}}
    surface = controller.Surface.from_arrays(Z, cm, hw)
    robot = controller.Robot(B.START[0], B.START[1], [1.0, 0.0, 0.0], cfg)
    ctl = controller.MPPI_Controller(surface, robot, cfg, FAR[0], FAR[1], 0.0)
    goals = [B.MAIN[0][1], FAR]
    res = ctl.run_batch([B.START, B.START], [(1.0, 0.0, 0.0)] * 2, goals, max_loops=12)
    ctl.engine.close()
    assert len(res) == 2
    s1, s2 = np.float32(ctl.std_dev_u1), np.float32(ctl.std_dev_u2)
    for e, r in enumerate(res):
        ref = _ref_b(256, 20, B.start_state(B.START, goals[e], s1=s1, s2=s2), 7 + e, 12)   # seeds: seed + e
        n = ref["steps"]
        assert r["loops"] == n and r["reached"] == ref["reached"]
        assert len(r["x"]) == n + 1 and len(r["lin_vel"]) == n
        assert (r["x"][0], r["y"][0], r["z"][0]) == (B.START[0], B.START[1], 0)
        np.testing.assert_array_equal(np.array(r["x"][1:], np.float32), ref["rows"][:, 0])
        np.testing.assert_array_equal(np.array(r["y"][1:], np.float32), ref["rows"][:, 1])
        np.testing.assert_array_equal(np.array(r["z"][1:], np.float32), ref["rows"][:, 2])
        np.testing.assert_array_equal(np.array(r["lin_vel"], np.float32), ref["rows"][:, 6])
        np.testing.assert_array_equal(np.array(r["ang_vel"], np.float32), ref["rows"][:, 7])
    assert res[0]["reached"] and res[0]["loops"] < 12 and res[1]["loops"] == 12
