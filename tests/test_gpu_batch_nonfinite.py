"""GPU: a batch with one episode whose pose or terrain is not finite: the other
episodes do not notice, and the bad one does what the oracle's loop does.

E = 4 episodes, K = 256, H = 12, 3 steps, on the scene of tests/nonfinite_refs.py, through Batch.run,
the device step and the tracked device step.  Episode BAD either gets a NaN pose (x and y) for its
second step, or runs on a DEM slot whose far part is NaN (part of its sampled fan dies, asserted on
the oracle).  Each case runs twice, once with that episode healthy:
  * the other three episodes' commands, plans, logs, states, flags, scores and metrics are bitwise equal;
  * the bad episode's equal the references (oracle.mppi_ref.mppi_step per step, tests/batch_refs.py's
    loop, the critics on its logged rows, mppi_amd.batch.path_metrics / path_length) with NaN == NaN;
  * its emitted command is finite, its u_opt is +0.0 in the step without a finite cost, and a pose that
    is not a number never counts as reached.
"""
import functools

import numpy as np
import pytest

import batch_refs as B
import helpers as hp
import nonfinite_refs as N
from oracle import mppi_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

F32 = np.float32
E, K, H, STEPS, BAD = 4, 256, 12, 3, 2
NP = 4 * H + 12
SEEDS = (31, 32, 33, 34)
GOAL = (15.0, 2.0)
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _scenes():
    """(the engine's scene, the scene of DEM slot 0: NaN from 0.42 m ahead of the bad episode's start,
    where the faster part of an H = 12 fan arrives)."""
    Z, Zp = N.base_dem(), N.patched_dem("nan", 0.42)
    Z.setflags(write=False)
    Zp.setflags(write=False)
    return hp.scene_for(Z, N.flat_costmap(), N.HW), hp.scene_for(Zp, N.flat_costmap(), N.HW)


def _engine():
    from mppi_amd import _lib
    eng = _lib.Engine(_lib.make_params(K, H), 0)
    hp.bind_scene(eng, _scenes()[0])
    return eng


@functools.lru_cache(maxsize=None)
def _table():
    """states[STEPS + 1][E][11]: poses no model produced, axis-aligned unit headings (exact under the
    oracle's renormalisation), the rovers rolling at about 1 m/s; episode BAD starts at the origin
    heading +x, where slot 0's patch lies ahead."""
    rng = np.random.default_rng(8)
    axes = np.array([[1, 0, 0], [0, -1, 0], [-1, 0, 0], [0, 1, 0]], F32)
    t = np.zeros((STEPS + 1, E, 11), F32)
    for i in range(STEPS + 1):
        for e in range(E):
            x, y = (0.05 * i, 0.0) if e == BAD else (-8.0 + 4.0 * e + rng.uniform(-1, 1), 3.0 + rng.uniform(-1, 1))
            h = axes[0] if e == BAD else axes[(i + e) % 4]
            t[i, e] = (x, y, h[0], h[1], h[2], rng.uniform(0.8, 1.1), rng.uniform(0.8, 1.1), GOAL[0], GOAL[1],
                       rng.uniform(0.4, 0.5), rng.uniform(0.4, 0.5))
    t.setflags(write=False)
    return t


def _variant_table(variant, healthy):
    t = _table().copy()
    if variant == "nan-pose" and not healthy:
        t[1, BAD, 0:2] = NAN
    return t


def _as_given(row):
    from mppi_amd.batch import to_mppi_state, unpack_states
    return to_mppi_state(unpack_states(np.asarray(row, F32)[None])[0])


def _open(eng, rows, variant, healthy):
    from mppi_amd import _lib
    batch = _lib.Batch(eng, E)
    if variant == "nan-dem":    # (the healthy twin holds the same slot with the engine's own heights)
        batch.set_dem(0, _scenes()[0 if healthy else 1].Z)
    for e in range(E):
        batch.set_episode(e, _as_given(rows[e]), SEEDS[e], dem=0 if (variant == "nan-dem" and e == BAD) else -1)
    return batch


def _oracle_steps(rows, seed, sc):
    """reference A of the device step: plans [n][4H + 12], the costs of every step, the last nominal."""
    p = R.Params(K=K, H=H, seed=seed)
    u1, u2 = np.zeros(H, F32), np.zeros(H, F32)
    plans, costs = [], []
    with np.errstate(all="ignore"):
        for i, r in enumerate(rows):
            S = R.State(x=float(r[0]), y=float(r[1]), heading=np.asarray(r[2:5], np.float64),
                        left_wheel_speed=float(r[5]), right_wheel_speed=float(r[6]), goal_x=float(r[7]),
                        goal_y=float(r[8]), std_dev_u1=float(r[9]), std_dev_u2=float(r[10]))
            o = R.mppi_step(p, sc, S, u1, u2, i)
            u1, u2 = o["u1_opt"], o["u2_opt"]
            plans.append(np.concatenate([o["u1_opt"], o["u2_opt"], o["v_opt"], o["w_opt"], o["traj_sim"][0],
                                         o["hv_sim"][0], o["lw_sim"][0], o["rw_sim"][0]]).astype(F32))
            costs.append(o["cost"])
    return np.array(plans, F32), costs, (u1, u2)


def _assert_scene_property(variant, costs):
    """On the oracle: the NaN pose kills its whole step and no other; the NaN DEM part of every step."""
    dead = [float((~np.isfinite(c)).mean()) for c in costs]
    if variant == "nan-pose":
        assert dead == [0.0, 1.0, 0.0], dead
    else:
        assert all(0.0 < d < 1.0 for d in dead), dead


def _bad_plan_checks(variant, plans_bad, want, tag):
    N.assert_same(f"{tag} plan", plans_bad, want)
    cmd = np.stack([plans_bad[:, 2 * H], plans_bad[:, 3 * H]], -1)
    assert np.isfinite(cmd).all(), f"{tag}: the emitted command is not finite"
    assert np.isfinite(plans_bad[:, :4 * H]).all(), f"{tag}: u_opt / lin_vel / ang_vel not finite"
    if variant == "nan-pose":
        assert np.array_equal(_bits(plans_bad[1, :2 * H]), np.zeros(2 * H, np.uint32)), f"{tag}: u_opt of the dead step"
        assert plans_bad[2, :2 * H].any()    # the next good pose recovers


# ================================================================== the device step
@pytest.mark.parametrize("variant", ["nan-pose", "nan-dem"])
def test_step_device_isolation(variant):
    import torch

    def run(healthy):
        table = _variant_table(variant, healthy)
        eng = _engine()
        try:
            batch = _open(eng, table[0], variant, healthy)
            cmds, plans = [], []
            for i in range(STEPS):
                cmd, plan = batch.step_device(torch.from_numpy(table[i].copy()).cuda())
                eng.sync()
                cmds.append(cmd.cpu().numpy())
                plans.append(plan.cpu().numpy())
            infos = [batch.episode(e) for e in range(E)]
            batch.close()
        finally:
            eng.close()
        return np.array(cmds), np.array(plans), infos

    sc = _scenes()[1 if variant == "nan-dem" else 0]
    want, costs, nominal = _oracle_steps(_variant_table(variant, False)[:STEPS, BAD], SEEDS[BAD], sc)
    _assert_scene_property(variant, costs)
    cmd_h, plan_h, info_h = run(True)
    cmd_b, plan_b, info_b = run(False)
    for e in range(E):
        if e == BAD:
            continue
        assert np.array_equal(_bits(cmd_b[:, e]), _bits(cmd_h[:, e])), f"cmd of episode {e}"
        assert np.array_equal(_bits(plan_b[:, e]), _bits(plan_h[:, e])), f"plan of episode {e}"
        for k in ("u1", "u2"):
            assert np.array_equal(_bits(info_b[e][k]), _bits(info_h[e][k])), f"nominal {k} of episode {e}"
    if variant == "nan-pose":    # (a dead part of the fan may leave the sparse optimum what it was; a dead step cannot)
        assert not np.array_equal(_bits(plan_b[:, BAD]), _bits(plan_h[:, BAD]))
    _bad_plan_checks(variant, plan_b[:, BAD], want, f"device step {variant}")
    assert np.array_equal(_bits(cmd_b[:, BAD]), _bits(np.stack([want[:, 2 * H], want[:, 3 * H]], -1)))
    assert np.array_equal(_bits(info_b[BAD]["u1"]), _bits(nominal[0]))
    assert np.array_equal(_bits(info_b[BAD]["u2"]), _bits(nominal[1]))


# ================================================================== the tracked device step
def _oracle_score(rows, origin, sc):
    """(cost, terms [4], collisions) of one logged path in the body-slope mode (lw = rw = traj)."""
    traj = np.ascontiguousarray(rows[None, :, 0:3], F32)
    v = np.ascontiguousarray(rows[None, :, 6], F32)
    p = R.Params(K=1, H=len(rows), horizon=0.045 * 2.0 * H)
    st = R.State(x=float(origin[0]), y=float(origin[1]), goal_x=float(origin[7]), goal_y=float(origin[8]))
    with np.errstate(all="ignore"):
        terms = np.stack(R.critic_terms(p, sc, st, traj, traj, traj, v), -1)[0]
        cost = R.critics(p, sc, st, traj, traj, traj, v)[0]
        col = int((R.costmap_at(sc, traj[:, :, 0], traj[:, :, 1]) > p.f("collision_threshold")).sum())
    return cost, terms, col


@pytest.mark.parametrize("variant", ["nan-pose", "nan-dem"])
def test_step_tracked_isolation(variant):
    """STEPS + 1 calls with a cap of STEPS rows: the last call ingests the last row and ends every run at
    the cap.  The bad episode's rows hold its NaN pose; its run is not `reached`."""
    import torch
    from mppi_amd.batch import path_length, path_metrics
    zs = (0.1 * np.arange((STEPS + 1) * E, dtype=F32)).reshape(STEPS + 1, E)

    def run(healthy):
        table = _variant_table(variant, healthy)
        eng = _engine()
        try:
            batch = _open(eng, table[0], variant, healthy)
            batch.set_tracking(max_steps=STEPS, runs_per_episode=1, keep_log=True, goal_tol=0.5, metrics=True)
            cmds, plans, dones = [], [], []
            for i in range(STEPS + 1):
                cmd, plan, done = batch.step_device(torch.from_numpy(table[i].copy()).cuda(),
                                                    z=torch.from_numpy(zs[i].copy()).cuda())
                eng.sync()
                cmds.append(cmd.cpu().numpy())
                plans.append(plan.cpu().numpy())
                dones.append(done.cpu().numpy())
            out = dict(cmd=np.array(cmds), plan=np.array(plans), done=np.array(dones),
                       logs=[batch.log(e) for e in range(E)], runs=[batch.runs(e) for e in range(E)],
                       reached=[batch.episode(e)["reached"] for e in range(E)], counts=list(batch.run_counts()))
            batch.close()
        finally:
            eng.close()
        return out

    sc = _scenes()[1 if variant == "nan-dem" else 0]
    table = _variant_table(variant, False)
    want, costs, _ = _oracle_steps(table[:STEPS, BAD], SEEDS[BAD], sc)
    _assert_scene_property(variant, costs)
    h, b = run(True), run(False)
    assert b["counts"] == [1] * E and (b["done"][:-1] == 0).all() and (b["done"][-1] == 2).all(), b["done"]
    assert np.array_equal(b["done"], h["done"])
    for e in range(E):
        if e == BAD:
            continue
        assert np.array_equal(_bits(b["cmd"][:, e]), _bits(h["cmd"][:, e])), f"cmd of episode {e}"
        assert np.array_equal(_bits(b["plan"][:, e]), _bits(h["plan"][:, e])), f"plan of episode {e}"
        assert np.array_equal(_bits(b["logs"][e]), _bits(h["logs"][e])), f"log of episode {e}"
        assert b["reached"][e] == h["reached"][e]
        for k, v in h["runs"][e].items():
            assert np.array_equal(np.ascontiguousarray(b["runs"][e][k]).view(np.uint8),
                                  np.ascontiguousarray(v).view(np.uint8)), f"runs[{k}] of episode {e}"
    # the bad episode: its steps, its log, its flags, its score and metrics
    _bad_plan_checks(variant, b["plan"][:STEPS, BAD], want, f"tracked step {variant}")
    rows = np.array([[table[i + 1, BAD, 0], table[i + 1, BAD, 1], zs[i + 1, BAD], *table[i + 1, BAD, 2:5],
                      *b["cmd"][i, BAD]] for i in range(STEPS)], F32)
    N.assert_same("log of the bad episode", b["logs"][BAD], rows)
    run_b = b["runs"][BAD]
    assert run_b["status"][0] == 2 and run_b["steps"][0] == run_b["rows"][0] == STEPS
    assert not run_b["reached"][0] and not b["reached"][BAD]
    cost, terms, col = _oracle_score(rows, table[0, BAD], _scenes()[0] if variant == "nan-pose" else sc)
    N.assert_same("score cost", run_b["cost"][:1], np.array([cost], F32))
    N.assert_same("score terms", run_b["terms"][0], terms)
    assert run_b["collisions"][0] == col
    N.assert_same("metrics", run_b["metrics"][0], path_metrics(rows))
    N.assert_same("length", run_b["length"][:1], np.array([path_length(rows)]))
    if variant == "nan-pose":    # (the far path-follow branch reads the last row only: the score stays finite)
        assert np.isnan(rows[0, 0:2]).all() and np.isfinite(rows[1:, 0:2]).all()


# ================================================================== Batch.run
@pytest.mark.parametrize("variant", ["nan-pose", "nan-dem"])
def test_run_isolation(variant):
    """Batch.run advances the states itself, so the NaN pose is set between two runs: run(1), then
    set_episode of episode BAD (the healthy twin sets a good pose there), then run(STEPS - 1).  With a NaN x
    and y the old goal test `!(|dx| > tol || |dy| > tol)` called the episode reached; it runs to the cap."""
    from mppi_amd import _lib
    from mppi_amd.batch import path_length, path_metrics
    table = _table()
    pol = _lib.make_policy(**B.RUN)

    def second_start(healthy):
        row = table[1, BAD].copy()
        if variant == "nan-pose" and not healthy:
            row[0:2] = NAN
        return row

    def run(healthy):
        eng = _engine()
        try:
            batch = _open(eng, table[0], variant, healthy)
            batch.run(1, "3d", pol)
            first = [batch.log(e) for e in range(E)]
            batch.set_episode(BAD, _as_given(second_start(healthy)), SEEDS[BAD],
                              dem=0 if variant == "nan-dem" else -1)
            batch.run(STEPS - 1, "3d", pol)
            out = dict(first=first, logs=[batch.log(e) for e in range(E)], infos=[batch.episode(e) for e in range(E)],
                       score=batch.score(metrics=True))
            batch.close()
        finally:
            eng.close()
        return out

    h, b = run(True), run(False)
    for e in range(E):
        if e == BAD:
            continue
        assert np.array_equal(_bits(b["first"][e]), _bits(h["first"][e])) and np.array_equal(_bits(b["logs"][e]), _bits(h["logs"][e]))
        ib, ih = b["infos"][e], h["infos"][e]
        assert bytes(ib["state"]) == bytes(ih["state"]) and ib["reached"] == ih["reached"]
        assert ib["steps_total"] == ih["steps_total"] == STEPS
        for k in ("u1", "u2"):
            assert np.array_equal(_bits(ib[k]), _bits(ih[k]))
        for k in ("cost", "terms", "collisions", "rows", "metrics"):
            assert np.array_equal(np.ascontiguousarray(b["score"][k][e]).view(np.uint8),
                                  np.ascontiguousarray(h["score"][k][e]).view(np.uint8)), f"score[{k}] of episode {e}"
    # the bad episode against tests/batch_refs.py's loop on the oracle
    sc = _scenes()[1 if variant == "nan-dem" else 0]
    row = second_start(False)
    st = dict(x=row[0], y=row[1], heading=np.asarray(row[2:5], np.float64), wl=row[5], wr=row[6], gx=row[7], gy=row[8],
              s1=row[9], s2=row[10])
    _, costs, _ = _oracle_steps([row], SEEDS[BAD], sc)
    dead = float((~np.isfinite(costs[0])).mean())
    assert dead == 1.0 if variant == "nan-pose" else 0.0 < dead < 1.0, dead
    with np.errstate(all="ignore"):
        ref = B.oracle_loop(K, H, sc, st, SEEDS[BAD], STEPS - 1)
    assert ref["steps"] == STEPS - 1 and not ref["reached"]
    info = b["infos"][BAD]
    assert info["steps_last_run"] == ref["steps"] and info["reached"] == ref["reached"]
    got_rows = b["logs"][BAD]
    N.assert_same("log rows", got_rows, ref["rows"])
    s = info["state"]
    final = np.array([s.x, s.y, *s.heading, s.left_wheel_speed, s.right_wheel_speed, s.goal_x, s.goal_y, s.std_dev_u1,
                      s.std_dev_u2], F32)
    N.assert_same("final state", final, ref["final"])
    N.assert_same("nominal u1", info["u1"], ref["u1"])
    N.assert_same("nominal u2", info["u2"], ref["u2"])
    assert np.isfinite(got_rows[:, 6:8]).all(), "the emitted command is not finite"
    assert np.isfinite(info["u1"]).all() and np.isfinite(info["u2"]).all()
    if variant == "nan-pose":
        assert np.isnan(got_rows[:, 0]).all() and not info["u1"].any() and not info["u2"].any()
    cost, terms, col = _oracle_score(got_rows, row, sc)
    N.assert_same("score cost", b["score"]["cost"][BAD:BAD + 1], np.array([cost], F32))
    N.assert_same("score terms", b["score"]["terms"][BAD], terms)
    assert b["score"]["collisions"][BAD] == col and b["score"]["rows"][BAD] == STEPS - 1
    N.assert_same("metrics", b["score"]["metrics"][BAD], path_metrics(got_rows))
