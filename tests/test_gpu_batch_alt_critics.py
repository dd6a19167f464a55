"""GPU: the critic sets of a batch's variant rows (mppi_batch_set_variant_critics).

Contract: every step of an episode, task or device step that holds a variant with a critic row is
bitwise the mppi_step of a context with the variant's params after mppi_set_critics(row); an episode
without a variant runs with the context's set.  K = 256, H = 20, 8 steps, the C3 scene; reference A
is the oracle loop under the wrapper of tests/alt_critics_refs.py, reference B a fresh engine with
set_critics stepped from the host.
"""
import functools

import numpy as np
import pytest

import alt_critics_refs as A
import batch_refs as B
import batch_variant_refs as V

pytestmark = pytest.mark.gpu

F32 = np.float32
AHEAD = (1.0, 0.0, 0.0)
WHEELS = dict(slope="wheels", w_orientation=0.0)
BODY = dict(slope="body", w_orientation=0.0)
ORIENT = dict(slope="wheels", w_orientation=1e5)
# name -> (projection, critic row or None: no variant, heading, the default twin, rows that must differ)
EPISODES = {
    "2d_wheels": ("2d", WHEELS, AHEAD, None, 0),
    "2d_body": ("2d", BODY, AHEAD, "2d_wheels", 8),
    "3d_body": ("3d", BODY, AHEAD, "3d_default", 8),
    "3d_orientation": ("3d", ORIENT, A.BACK, "3d_default_back", 3),
    "context_body": ("3d", None, AHEAD, "3d_default", 8),       # runs with the context's set: body
    "3d_default": ("3d", WHEELS, AHEAD, None, 0),
    "3d_default_back": ("3d", WHEELS, A.BACK, None, 0),
}
NAMES = list(EPISODES)
CONTEXT = BODY


def _crit(name):
    return EPISODES[name][1] or CONTEXT


def _variants():
    """One variant per episode that holds one, as dicts with the critic keys (Batch.set_variants splits them)."""
    from mppi_amd.batch import variant_dict
    rows, index = [], {}
    for n in NAMES:
        proj, crit, _, _, _ = EPISODES[n]
        if crit is not None:
            index[n] = len(rows)
            rows.append(dict(variant_dict(proj), **crit))
    return rows, index


def _state(name):
    return V.mppi_state(B.start_state(B.START, A.FAR, EPISODES[name][2]))


@functools.lru_cache(maxsize=None)
def _ref_a(name):
    return A.loop(EPISODES[name][0], _crit(name), EPISODES[name][2])


def _engine():
    eng = V.make_engine(A.K1, A.H1)
    eng.set_critics(**CONTEXT)
    return eng


@functools.lru_cache(maxsize=None)
def _batch_run():
    from mppi_amd import _lib
    eng = _engine()
    try:
        batch = _lib.Batch(eng, len(NAMES))
        rows, index = _variants()
        batch.set_variants(rows)
        for e, n in enumerate(NAMES):
            batch.set_episode(e, _state(n), A.SEED_LOOP, index.get(n, -1))
        batch.run(A.STEPS_LOOP, "3d", _lib.make_policy(**B.RUN))
        out = {n: V.collect(batch, e) for e, n in enumerate(NAMES)}
        scores = batch.score()
        origins = [V.origin_state(B.START[0], B.START[1], A.FAR[0], A.FAR[1])] * len(NAMES)
        V.check_scores(scores, eng, [out[n]["rows"] for n in NAMES], origins, "body context")
        batch.close()
    finally:
        eng.close()
    return out, scores


@pytest.mark.parametrize("name", NAMES)
def test_episode_matches_both_references(name):
    got = _batch_run()[0][name]
    assert got["steps"] == A.STEPS_LOOP
    V.same(got, _ref_a(name), f"{name} vs A")
    V.same(got, A.engine_loop(EPISODES[name][0], _crit(name), EPISODES[name][2]), f"{name} vs B")


@pytest.mark.parametrize("name", [n for n in NAMES if EPISODES[n][3]])
def test_episode_differs_from_its_default_twin(name):
    got = _batch_run()[0]
    twin, least = EPISODES[name][3], EPISODES[name][4]
    n = A.rows_changed(got[name], got[twin])
    print(f"{name}: {n} of {A.STEPS_LOOP} rows differ from {twin}")
    assert n >= least


def test_score_uses_the_context_set():
    """Batch.score() on the body context equals score_one per episode (checked in the run above); with
    an orientation weight on the context the log scorer's cost has the term."""
    from mppi_amd import _lib
    out, scores = _batch_run()
    eng = V.make_engine(A.K1, A.H1)
    try:
        rows = out["3d_default_back"]["rows"]
        origin = V.origin_state(B.START[0], B.START[1], A.FAR[0], A.FAR[1])
        plain = V.score_one(eng, rows, origin)
        e = NAMES.index("3d_default_back")
        assert F32(plain["cost"]).view(np.uint32) == F32(scores["cost"][e]).view(np.uint32)   # a log is a body path
        eng.set_critics("wheels", 1000.0)
        with_term = V.score_one(eng, rows, origin)
        assert np.array_equal(np.asarray(with_term["terms"]), np.asarray(plain["terms"]))
        st = A.R.State(x=B.START[0], y=B.START[1], goal_x=A.FAR[0], goal_y=A.FAR[1])
        po = A.orientation(st, rows[None, :, 0:3])
        assert po[0] != 0
        t5 = np.concatenate([np.asarray(plain["terms"], F32), po])[None]
        p = eng.params
        want = A.recombine(t5, [p.w_path, p.w_slope, p.w_speed, p.w_obstacle], 1000.0)
        assert F32(with_term["cost"]).view(np.uint32) == want.view(np.uint32)[0]
        # the batch's log scorer with the same context set
        batch = _lib.Batch(eng, 1)
        batch.set_episode(0, _state("3d_default_back"), A.SEED_LOOP)
        batch.run(A.STEPS_LOOP, "3d", _lib.make_policy(**B.RUN))
        V.check_scores(batch.score(), eng, [batch.log(0)], [origin], "orientation context")
        batch.close()
    finally:
        eng.close()


def test_tasks_run_with_their_critic_rows():
    from mppi_amd import _lib
    eng = _engine()
    try:
        batch = _lib.Batch(eng, 3)          # fewer lanes than tasks: lanes change critic rows as they claim
        rows, index = _variants()
        batch.set_variants(rows)
        batch.set_tasks([_lib.make_task(_state(n), A.SEED_LOOP, A.STEPS_LOOP, index.get(n, -1)) for n in NAMES])
        done = 0
        while done < len(NAMES):
            done, steps = batch.run_tasks(100, "3d", _lib.make_policy(**B.RUN))
            assert steps > 0 or done == len(NAMES)
        for i, n in enumerate(NAMES):
            info = batch.task(i)
            ref = _ref_a(n)
            assert info["steps"] == ref["steps"], n
            got = batch.task_log(i)
            assert np.array_equal(got.view(np.uint32), ref["rows"].view(np.uint32)), n
        batch.close()
    finally:
        eng.close()


def test_step_device_matches_engine_step():
    import torch
    from mppi_amd import _lib
    from mppi_amd.batch import pack_states, state_dict
    H = A.H1
    eng = _engine()
    try:
        batch = _lib.Batch(eng, len(NAMES))
        rows, index = _variants()
        batch.set_variants(rows)
        for e, n in enumerate(NAMES):
            batch.set_episode(e, _state(n), A.SEED_LOOP, index.get(n, -1))
        states = torch.as_tensor(pack_states([state_dict(B.START[0], B.START[1], EPISODES[n][2], 0.0, 0.0, A.FAR[0],
                                                         A.FAR[1], 0.25, 0.25) for n in NAMES])).cuda()
        cmd, plan = batch.step_device(states, proj="3d")
        eng.sync()
        plan = plan.cpu().numpy()
        batch.close()
    finally:
        eng.close()
    for e, n in enumerate(NAMES):
        one = V.make_engine(A.K1, A.H1, seed=A.SEED_LOOP)
        try:
            one.set_critics(**_crit(n))
            one.set_state(_state(n))
            o = one.step(EPISODES[n][0], 0)
        finally:
            one.close()
        want = np.concatenate([o["u1_opt"], o["u2_opt"], o["lin_vel"], o["ang_vel"], o["traj_sim"][0],
                               o["heading_sim"][0], o["left_wheel_sim"][0], o["right_wheel_sim"][0]]).astype(F32)
        assert plan[e].shape == (4 * H + 12,)
        assert np.array_equal(plan[e].view(np.uint32), want.view(np.uint32)), n
