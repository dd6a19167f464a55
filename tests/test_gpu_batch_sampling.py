"""GPU: the sampling plans of a batch's variant rows (mppi_batch_set_variant_sampling).

Contract: every step of an episode, task, device step or tracked run that holds a variant with a
sampling row is bitwise the mppi_step of a context after mppi_set_sampling(row); an episode without a
variant runs with the context's plan.  K = 300 (two ragged leaves), H = 5 (odd), four steps on the C3
scene; reference A is the oracle loop on injected controls (tests/sampling_refs.py), reference B a
fresh engine with set_sampling stepped from the host (the tests/batch_refs.py pattern).
"""
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V
import helpers as hp
import sampling_refs as SR

pytestmark = pytest.mark.gpu

F32 = np.float32
K, H, STEPS = 300, 5, 4
NP = 4 * H + 12
AHEAD = (1.0, 0.0, 0.0)
CONTEXT = SR.NOM_ANTI
ANTI_HALF = dict(antithetic=True, nominal=False, beta=0.5)
# name -> (projection, plan or None: no variant, seed)
EPISODES = {
    "nominal": ("3d", SR.NOMINAL, 11),
    "combined_2d": ("2d", SR.ALL, 12),
    "anti_beta": ("3d", ANTI_HALF, 13),
    "beta": ("3d", SR.BETA, 14),
    "context": ("3d", None, 15),
}
NAMES = list(EPISODES)


def _plan(name):
    return EPISODES[name][1] or CONTEXT


def _variants():
    """One variant per episode that holds one, as dicts with the sampling keys (Batch.set_variants splits them)."""
    from mppi_amd.batch import variant_dict
    rows, index = [], {}
    for n in NAMES:
        proj, plan, _ = EPISODES[n]
        if plan is not None:
            index[n] = len(rows)
            rows.append(dict(variant_dict(proj), antithetic=plan["antithetic"], nominal=plan["nominal"],
                             noise_beta=plan["beta"]))
    return rows, index


def _start():
    return B.start_state(B.START, SR.FAR, AHEAD)


def _engine(seed=42, plan=CONTEXT):
    eng = V.make_engine(K, H, seed=seed)
    eng.set_sampling(**plan)
    return eng


@functools.lru_cache(maxsize=None)
def _ref_a(name):
    proj, _, seed = EPISODES[name]
    return SR.oracle_loop(K, H, _start(), seed, STEPS, _plan(name), proj)


@functools.lru_cache(maxsize=None)
def _ref_b(name):
    proj, _, seed = EPISODES[name]
    Z, hw, cm = hp.c3_scene()
    return B.engine_loop(K, H, Z, hw, cm, _start(), seed, STEPS, proj,
                         make_engine=lambda s: _engine(s, _plan(name)))


def _open(eng, lanes=None):
    from mppi_amd import _lib
    batch = _lib.Batch(eng, lanes or len(NAMES))
    rows, index = _variants()
    batch.set_variants(rows)
    return batch, index


@functools.lru_cache(maxsize=None)
def _batch_run():
    from mppi_amd import _lib
    eng = _engine()
    try:
        batch, index = _open(eng)
        for e, n in enumerate(NAMES):
            batch.set_episode(e, V.mppi_state(_start()), EPISODES[n][2], index.get(n, -1))
        batch.run(STEPS, "3d", _lib.make_policy(**B.RUN))
        out = {n: V.collect(batch, e) for e, n in enumerate(NAMES)}
        batch.close()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_episode_matches_both_references(name):
    got = _batch_run()[name]
    assert got["steps"] == STEPS
    V.same(got, _ref_a(name), f"{name} vs A")
    V.same(got, _ref_b(name), f"{name} vs B")


def test_plans_are_not_ignored():
    """(each episode's log differs from the same episode under the default plan)"""
    Z, hw, cm = hp.c3_scene()
    for n in NAMES:
        proj, _, seed = EPISODES[n]
        dflt = B.engine_loop(K, H, Z, hw, cm, _start(), seed, STEPS, proj, make_engine=lambda s: _engine(s, SR.DEFAULT))
        assert V.differ(_batch_run()[n], dflt) >= 1, n


def test_tasks_run_with_their_plan_rows():
    """Six tasks on two lanes: the lanes change plan rows (and generator forms) as they claim."""
    from mppi_amd import _lib
    tasks = NAMES + ["beta"]
    eng = _engine()
    try:
        batch, index = _open(eng, lanes=2)
        batch.set_tasks([_lib.make_task(V.mppi_state(_start()), EPISODES[n][2], STEPS, index.get(n, -1)) for n in tasks])
        done = 0
        while done < len(tasks):
            done, steps = batch.run_tasks(100, "3d", _lib.make_policy(**B.RUN))
            assert steps > 0 or done == len(tasks)
        for i, n in enumerate(tasks):
            ref = _ref_a(n)
            assert batch.task(i)["steps"] == ref["steps"], n
            assert np.array_equal(batch.task_log(i).view(np.uint32), ref["rows"].view(np.uint32)), n
        batch.close()
    finally:
        eng.close()


def _pack(states):
    from mppi_amd.batch import pack_states
    return pack_states(states)


def _plan_row(o):
    row0 = [np.asarray(o[n], F32).reshape(-1, 3)[0] for n in ("traj_sim", "heading_sim", "left_wheel_sim",
                                                                 "right_wheel_sim")]
    return np.concatenate([np.asarray(o[n], F32) for n in ("u1_opt", "u2_opt", "lin_vel", "ang_vel")] + row0)


def test_step_device_matches_engine_steps():
    """Two device steps from given states (the second from a state no model produced)."""
    import torch
    from mppi_amd.batch import state_dict, to_mppi_state
    given = [state_dict(B.START[0], B.START[1], AHEAD, 0.0, 0.0, SR.FAR[0], SR.FAR[1], 0.25, 0.25),
             state_dict(B.START[0] + 0.4, B.START[1] - 0.3, (0.0, 1.0, 0.0), 0.3, 0.5, SR.FAR[0], SR.FAR[1], 0.3, 0.45)]
    eng = _engine()
    try:
        batch, index = _open(eng)
        for e, n in enumerate(NAMES):
            batch.set_episode(e, to_mppi_state(given[0]), EPISODES[n][2], index.get(n, -1))
        plans = []
        for s in given:
            cmd, plan = batch.step_device(torch.as_tensor(_pack([s] * len(NAMES))).cuda(), proj="3d")
            eng.sync()
            plans.append(plan.cpu().numpy())
        batch.close()
    finally:
        eng.close()
    for e, n in enumerate(NAMES):
        one = _engine(EPISODES[n][2], _plan(n))
        try:
            for i, s in enumerate(given):
                one.set_state(to_mppi_state(s))
                want = _plan_row(one.step(EPISODES[n][0], i))
                assert plans[i][e].shape == (NP,)
                assert np.array_equal(plans[i][e].view(np.uint32), want.view(np.uint32)), (n, i)
        finally:
            one.close()


def test_tracked_run_reproduces_batch_run():
    """The controller's own model as the plant of a tracked run: its log is Batch.run's, bit for bit."""
    import torch
    from mppi_amd.batch import advance_state, from_mppi_state, state_dict
    E = len(NAMES)
    start = state_dict(B.START[0], B.START[1], AHEAD, 0.0, 0.0, SR.FAR[0], SR.FAR[1], 0.25, 0.25)
    eng = _engine()
    try:
        radius = float(eng.params.robot_radius)
        batch, index = _open(eng)
        for e, n in enumerate(NAMES):
            batch.set_episode(e, V.mppi_state(_start()), EPISODES[n][2], index.get(n, -1))
        batch.set_tracking(max_steps=STEPS, runs_per_episode=1, keep_log=True, goal_tol=B.RUN["goal_tol"])
        states, z = [dict(start) for _ in range(E)], np.zeros(E, F32)
        for _ in range(STEPS + 1):
            cmd, plan, done = batch.step_device(torch.as_tensor(_pack(states)).cuda(), z=torch.as_tensor(z).cuda())
            eng.sync()
            cmd, plan, done = cmd.cpu().numpy(), plan.cpu().numpy(), done.cpu().numpy()
            for e in np.nonzero(done == 0)[0]:
                states[e], _ = advance_state(states[e], plan[e, 4 * H:4 * H + 3], plan[e, 4 * H + 3:4 * H + 6],
                                             cmd[e, 0], cmd[e, 1], radius, B.RUN)
                z[e] = plan[e, 4 * H + 2]
        assert (done == 2).all()                       # every run ended at the cap
        for e, n in enumerate(NAMES):
            want = _batch_run()[n]["rows"]
            assert np.array_equal(batch.log(e).view(np.uint32), want.view(np.uint32)), n
        batch.close()
    finally:
        eng.close()
