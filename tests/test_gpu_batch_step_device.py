"""GPU: the batch's device-resident step (include/mppi.h mppi_batch_step_device).

The plant is the caller's: states come from device memory, the command and the plan go back there.
Every step of every episode is compared bit for bit with
  reference A  oracle.mppi_ref.mppi_step (CPU)
  reference B  a fresh Engine per episode with set_state (the heading as given) + step(proj, i)
on the scene of tests/test_gpu_batch.py (helpers.c3_scene()), H = 20, K = 256 unless stated.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V

pytestmark = pytest.mark.gpu

F32 = np.float32
H = 20
NP = 4 * H + 12
FAR = (65.0, 10.0)
SENTINEL = -12345.0
MPPI_EINVAL, MPPI_ESTATE = -1, -3


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _engine(K=256, Z=None, cm=None, **params):
    from helpers import c3_scene
    from mppi_amd import _lib
    Z0, hw, cm0 = c3_scene()
    eng = _lib.Engine(_lib.make_params(K, H, **params), 0)
    eng.set_dem(Z0 if Z is None else Z, hw)
    eng.set_costmap(cm0 if cm is None else cm, hw)
    return eng


def _as_given(row):
    """The MppiState of one row of a states array: every field as given, the heading too."""
    from mppi_amd.batch import to_mppi_state, unpack_states
    return to_mppi_state(unpack_states(np.asarray(row, F32)[None])[0])


def _plan_of(o):
    """The plan row a step's outputs make: u1_opt, u2_opt, lin_vel, ang_vel, then row 0 of the four paths."""
    row0 = [np.asarray(o[n], F32).reshape(-1, 3)[0] for n in ("traj_sim", "heading_sim", "left_wheel_sim",
                                                                 "right_wheel_sim")]
    return np.concatenate([np.asarray(o[n], F32) for n in ("u1_opt", "u2_opt", "lin_vel", "ang_vel")] + row0)


def ref_b(rows, seed, K=256, proj="3d", params=None, Z=None, cm=None):
    """Reference B: a fresh engine (seed, K, params, scene) fed `rows` [n][11], one step each from step
    index 0.  Returns (plans [n][4H + 12], the nominal sequence after the last step)."""
    eng = _engine(K, Z, cm, seed=seed, **{k: float(v) for k, v in (params or {}).items()})
    try:
        plans = []
        for i, row in enumerate(rows):
            eng.set_state(_as_given(row))
            plans.append(_plan_of(eng.step(proj, i)))
        u1, u2 = eng.get_nominal()
    finally:
        eng.close()
    return np.array(plans, F32).reshape(len(rows), NP), (np.asarray(u1, F32), np.asarray(u2, F32))


def ref_a(rows, seed, K=256, proj="3d"):
    """Reference A: the same on the CPU oracle (headings that normalise to themselves only)."""
    from helpers import c3_scene, oracle_scene
    from oracle import mppi_ref as R
    p = R.Params(K=K, H=H, seed=seed)
    sc = oracle_scene(*c3_scene())
    u1, u2 = np.zeros(H, F32), np.zeros(H, F32)
    plans = []
    for i, r in enumerate(rows):
        S = R.State(x=float(r[0]), y=float(r[1]), heading=np.asarray(r[2:5], np.float64), left_wheel_speed=float(r[5]),
                    right_wheel_speed=float(r[6]), goal_x=float(r[7]), goal_y=float(r[8]), std_dev_u1=float(r[9]),
                    std_dev_u2=float(r[10]))
        assert np.array_equal(S.heading_f32(), np.asarray(r[2:5], F32))
        o = R.mppi_step(p, sc, S, u1, u2, i, proj)
        u1, u2 = o["u1_opt"], o["u2_opt"]
        plans.append(np.concatenate([o["u1_opt"], o["u2_opt"], o["v_opt"], o["w_opt"], o["traj_sim"][0], o["hv_sim"][0],
                                     o["lw_sim"][0], o["rw_sim"][0]]).astype(F32))
    return np.array(plans, F32), (np.asarray(u1, F32), np.asarray(u2, F32))


def _cmd_of(plans):
    return np.stack([plans[..., 2 * H], plans[..., 3 * H]], -1)


def _same_step(cmd, plan, want_plan, tag):
    assert np.array_equal(_bits(plan), _bits(want_plan)), f"plan {tag}"
    assert np.array_equal(_bits(cmd), _bits(_cmd_of(want_plan))), f"cmd {tag}"


def _same_nominal(batch, e, nominal, tag):
    info = batch.episode(e)
    assert np.array_equal(_bits(info["u1"]), _bits(nominal[0])), f"nominal u1 {tag}"
    assert np.array_equal(_bits(info["u2"]), _bits(nominal[1])), f"nominal u2 {tag}"
    return info


def _state_row(info):
    s = info["state"]
    return np.array([s.x, s.y, s.heading[0], s.heading[1], s.heading[2], s.left_wheel_speed, s.right_wheel_speed,
                     s.goal_x, s.goal_y, s.std_dev_u1, s.std_dev_u2], F32)


def _table(n, E, seed, near=None):
    """A fixed table states[n][E][11] about batch_refs.START: positions within a metre of it, unit
    headings (axis-aligned for episodes 0 and 1: exact under the oracle's renormalisation), wheel
    speeds, the far goal, sigmas in [0.25, 0.5).  Episode `near` keeps a goal 0.9 to 1.5 m away: inside
    the horizon of 1.8 m (the other path-follow branch) and inside 2 m (speed_on = 0)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, E, 11), F32)
    axes = np.array([[1, 0, 0], [0, -1, 0], [-1, 0, 0], [0, 1, 0]], F32)
    for i in range(n):
        for e in range(E):
            x, y = B.START[0] + rng.uniform(-1, 1), B.START[1] + rng.uniform(-1, 1)
            if e < 2:
                h = axes[(i + e) % 4]
            else:
                a = rng.uniform(0, 2 * np.pi)
                h = np.array([np.cos(a), np.sin(a), 0.0])
                h = (h / np.linalg.norm(h)).astype(F32)
            gx, gy = FAR
            if e == near:
                b = rng.uniform(0, 2 * np.pi)
                d = rng.uniform(0.9, 1.5)
                gx, gy = x + d * np.cos(b), y + d * np.sin(b)
            t[i, e] = (x, y, h[0], h[1], h[2], rng.uniform(0, 1), rng.uniform(0, 1), gx, gy, rng.uniform(0.25, 0.5),
                       rng.uniform(0.25, 0.5))
    return t


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _sentinels(torch, E):
    """cmd and plan filled with the sentinel (the fill has run before the engine's stream can write them)."""
    cmd = torch.full((E, 2), SENTINEL, dtype=torch.float32, device="cuda")
    plan = torch.full((E, NP), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return cmd, plan


def _step(torch, batch, rows, **kw):
    """One step_device from a host table, then the wait for the engine's own stream (torch's streams do
    not order with it): (cmd, plan) as ndarrays."""
    states = _dev(torch, rows)
    cmd, plan = batch.step_device(states, **kw)
    batch.engine.sync()
    return cmd.cpu().numpy(), plan.cpu().numpy()


def _open(eng, rows, seeds, **per_episode):
    """A Batch with episode e set at rows[e] with seeds[e]; per_episode: lists of set_episode's other arguments."""
    from mppi_amd import _lib
    batch = _lib.Batch(eng, len(rows))
    for e, (row, seed) in enumerate(zip(rows, seeds)):
        if seed is not None:
            batch.set_episode(e, _as_given(row), seed, **{k: v[e] for k, v in per_episode.items()})
    return batch


# ---- 1. given states ----
GIVEN_SEEDS = (21, 22, 23, 24, 25)
GIVEN_K = (256, 256, 256, 256, 300)


@functools.lru_cache(maxsize=None)
def _given():
    return _table(6, 5, 2024, near=3)


def test_given_states_are_stepped_bitwise():
    """E = 5, 6 steps from a table no model produced: cmd and plan are reference B's for all five and
    reference A's for two; one episode near its goal, one with K_e = 300 of a context K = 512."""
    torch = _gpu()
    table = _given()
    n, E = table.shape[:2]
    horizon = 0.045 * 2.0 * H
    dist = np.hypot(table[..., 7] - table[..., 0], table[..., 8] - table[..., 1])
    assert (dist[:, 3] < horizon).all() and (dist[:, 3] < 2.0).all() and (dist[:, [0, 1, 2, 4]] > horizon).all()
    eng = _engine(512)
    try:
        batch = _open(eng, table[0], GIVEN_SEEDS, trajectories=list(GIVEN_K))
        cmds, plans = [], []
        for i in range(n):
            cmd, plan = _step(torch, batch, table[i])
            cmds.append(cmd)
            plans.append(plan)
        cmds, plans = np.array(cmds), np.array(plans)
        # every row differs from the model's own next state: the feedback is the table's
        assert (np.abs(plans[:-1, :, 4 * H:4 * H + 2] - table[1:, :, 0:2]) > 1e-3).any(axis=-1).all()
        for e in range(E):
            want, nominal = ref_b(table[:, e], GIVEN_SEEDS[e], GIVEN_K[e])
            _same_step(cmds[:, e], plans[:, e], want, f"episode {e} against reference B")
            info = _same_nominal(batch, e, nominal, f"episode {e}")
            assert info["steps_total"] == n and info["steps_last_run"] == 0
            assert np.array_equal(_bits(_state_row(info)), _bits(table[-1, e])), f"record of episode {e}"
        for e in (0, 1):
            want, nominal = ref_a(table[:, e], GIVEN_SEEDS[e], GIVEN_K[e])
            _same_step(cmds[:, e], plans[:, e], want, f"episode {e} against reference A")
            _same_nominal(batch, e, nominal, f"episode {e} against reference A")
        batch.close()
    finally:
        eng.close()


# ---- 2. the plant on the device ----
def _unicycle(torch, states, cmd, dt=0.045, radius=1.2):
    """A trivial plant in tensor operations, in place: the pose integrated from (v, w), the wheel
    speeds a real platform would report, the Isaac loop's sigmas from the measured w."""
    v, w = cmd[:, 0], cmd[:, 1]
    hx, hy = states[:, 2].clone(), states[:, 3].clone()
    c, s = torch.cos(w * dt), torch.sin(w * dt)
    states[:, 0] += v * hx * dt
    states[:, 1] += v * hy * dt
    nx, ny = c * hx - s * hy, s * hx + c * hy
    norm = torch.sqrt(nx * nx + ny * ny)
    states[:, 2] = nx / norm
    states[:, 3] = ny / norm
    states[:, 5] = 0.9 * (v - w * radius / 2)      # (a plant that does not track the command exactly)
    states[:, 6] = 0.9 * (v + w * radius / 2)
    states[:, 9] = torch.clamp(0.25 - w * w / 3.0, min=0.25)
    states[:, 10] = torch.clamp(0.25 + w * w / 3.0, min=0.25)


@pytest.mark.parametrize("bind", ["before_create", "after_set_episode"])
def test_plant_on_the_device_without_host_synchronisation(bind):
    """E = 3, 8 steps: the states come from a torch unicycle integrated from cmd on the engine's stream,
    a non-default torch stream bound with set_stream (before the batch exists, or after its episodes are
    set), with no host synchronisation until the end; the recorded states replayed through reference B
    give the same bits."""
    torch = _gpu()
    E, n, seeds = 3, 8, (31, 32, 33)
    start = _table(1, E, 77)[0]
    stream = torch.cuda.Stream()
    eng = _engine()
    try:
        if bind == "before_create":
            eng.set_stream(stream.cuda_stream)
        batch = _open(eng, start, seeds)
        if bind == "after_set_episode":
            eng.set_stream(stream.cuda_stream)
        host = torch.as_tensor(start).pin_memory()
        with torch.cuda.stream(stream):
            states = host.to("cuda", non_blocking=True)
            seen = torch.empty((n, E, 11), dtype=torch.float32, device="cuda")
            cmds = torch.empty((n, E, 2), dtype=torch.float32, device="cuda")
            plans = torch.empty((n, E, NP), dtype=torch.float32, device="cuda")
            cmd, plan = _sentinels(torch, E)
            for i in range(n):
                seen[i].copy_(states)
                batch.step_device(states, cmd=cmd, plan=plan)
                cmds[i].copy_(cmd)
                plans[i].copy_(plan)
                _unicycle(torch, states, cmd)
        stream.synchronize()
        seen, cmds, plans = seen.cpu().numpy(), cmds.cpu().numpy(), plans.cpu().numpy()
        assert (seen[1:, :, 0:2] != seen[:-1, :, 0:2]).any(axis=-1).all()     # the plant moved every rover
        for e in range(E):
            want, nominal = ref_b(seen[:, e], seeds[e])
            _same_step(cmds[:, e], plans[:, e], want, f"episode {e}")
            _same_nominal(batch, e, nominal, f"episode {e}")
        batch.close()
    finally:
        eng.close()


# ---- 3. the controller's own model as the plant ----
def test_own_model_fed_back_reproduces_batch_run():
    """advance_state applied on the host to plan's row 0 and cmd, fed back through step_device, gives the
    log rows and the final nominal sequence of Batch.run for batch_refs.MAIN (10 steps)."""
    torch = _gpu()
    from mppi_amd import _lib
    from mppi_amd.batch import advance_state, from_mppi_state, is_active, pack_states, state_dict
    n, E = 10, len(B.MAIN)
    starts = [state_dict(s[0], s[1], (1.0, 0.0, 0.0), 0.0, 0.0, g[0], g[1]) for s, g, _, _ in B.MAIN]
    seeds = [m[2] for m in B.MAIN]
    ks = [m[3] for m in B.MAIN]
    eng = _engine(512)
    try:
        radius = float(eng.params.robot_radius)
        run = _open(eng, pack_states(starts), seeds, trajectories=ks)
        run.run(n, "3d", _lib.make_policy(**B.RUN))
        dev = _open(eng, pack_states(starts), seeds, trajectories=ks)
        states, rows = list(starts), [[] for _ in range(E)]
        for _ in range(n):
            mask = np.array([is_active(s, B.RUN) for s in states], np.int32)
            if not mask.any():
                break
            cmd, plan = _step(torch, dev, pack_states(states), mask=_dev(torch, mask))
            for e in np.nonzero(mask)[0]:
                states[e], row = advance_state(states[e], plan[e, 4 * H:4 * H + 3], plan[e, 4 * H + 3:4 * H + 6],
                                               cmd[e, 0], cmd[e, 1], radius, B.RUN)
                rows[e].append(row)
        assert [len(r) for r in rows] == [run.episode(e)["steps_last_run"] for e in range(E)]
        assert len(rows[3]) == 0 and len(rows[4]) == n        # inside the tolerance from the start; to the cap
        for e in range(E):
            got, want = run.episode(e), dev.episode(e)
            assert np.array_equal(_bits(np.array(rows[e], F32).reshape(-1, 8)), _bits(run.log(e))), f"rows of {e}"
            assert np.array_equal(_bits(got["u1"]), _bits(want["u1"])), f"nominal u1 of {e}"
            assert np.array_equal(_bits(got["u2"]), _bits(want["u2"])), f"nominal u2 of {e}"
            assert got["steps_total"] == want["steps_total"] == len(rows[e])
            assert np.array_equal(_bits(pack_states([from_mppi_state(got["state"])])), _bits(pack_states([states[e]])))
        run.close()
        dev.close()
    finally:
        eng.close()


# ---- 4. mask and reset ----
def test_mask_and_reset():
    """A masked episode's rows keep the sentinel, its step count and nominal sequence stay, and it goes on
    as if the masked call had not happened; a reset episode goes on as a fresh one with the new seed, or
    with its own seed without `seeds`; an episode never set does not run under mask = NULL."""
    torch = _gpu()
    E, seeds, NEW = 4, (41, 42, 43, None), 99
    t = _table(5, E, 404)
    eng = _engine()
    try:
        batch = _open(eng, t[0], seeds)
        i32, u64 = torch.int32, torch.int64
        calls = [dict(),
                 dict(mask=_dev(torch, [1, 0, 1, 1], i32)),
                 dict(),
                 dict(reset=_dev(torch, [0, 0, 1, 0], i32), seeds=_dev(torch, [5, 6, NEW, 7], u64)),
                 dict(reset=_dev(torch, [1, 0, 0, 1], i32))]
        cmds, plans = [], []
        for i, kw in enumerate(calls):
            before = batch.episode(1)
            cmd, plan = _sentinels(torch, E)
            cmd, plan = _step(torch, batch, t[i], cmd=cmd, plan=plan, **kw)
            cmds.append(cmd)
            plans.append(plan)
            if i == 1:      # episode 1 was masked out: nothing of it moved
                after = batch.episode(1)
                assert (cmds[1][1] == SENTINEL).all() and (plans[1][1] == SENTINEL).all()
                assert after["steps_total"] == before["steps_total"] == 1
                assert np.array_equal(_bits(after["u1"]), _bits(before["u1"]))
                assert np.array_equal(_bits(after["u2"]), _bits(before["u2"]))
                assert np.array_equal(_bits(_state_row(after)), _bits(t[0, 1]))
        cmds, plans = np.array(cmds), np.array(plans)
        # never set: no row written, no step counted, even when its reset flag is up
        assert (cmds[:, 3] == SENTINEL).all() and (plans[:, 3] == SENTINEL).all()
        assert batch.episode(3)["steps_total"] == 0

        def check(e, picks, want, nominal, tag):
            _same_step(cmds[picks, e], plans[picks, e], want, tag)
            if nominal is not None:
                _same_nominal(batch, e, nominal, tag)

        want, _ = ref_b(t[[0, 1, 2, 3], 0], seeds[0])
        check(0, [0, 1, 2, 3], want, None, "episode 0 before its reset")
        want, nominal = ref_b(t[[4], 0], seeds[0])
        check(0, [4], want, nominal, "episode 0 reset without seeds: its own seed, from step 0")
        want, nominal = ref_b(t[[0, 2, 3, 4], 1], seeds[1])
        check(1, [0, 2, 3, 4], want, nominal, "episode 1 around the masked call")
        want, _ = ref_b(t[[0, 1, 2], 2], seeds[2])
        check(2, [0, 1, 2], want, None, "episode 2 before its reset")
        want, nominal = ref_b(t[[3, 4], 2], NEW)
        check(2, [3, 4], want, nominal, "episode 2 reset with a new seed")
        assert [batch.episode(e)["steps_total"] for e in range(E)] == [1, 4, 2, 0]
        batch.close()
    finally:
        eng.close()


# ---- 5. variants and scenes in one call ----
def test_variants_and_scene_slots_in_one_call():
    """A 2D variant, a temperature variant, a DEM slot and a costmap slot in one batch (two rollout
    launches per step), each against reference B with the overridden params and the slot's scene."""
    torch = _gpu()
    from helpers import c3_scene
    Z, hw, cm = c3_scene()
    Z1 = np.ascontiguousarray(Z[::-1, ::-1])
    # the costmap slot: free ground but for a wall over x < -38.1, which the slot's episode faces at its
    # first state from 3 cm away (every rollout crosses it, the slow ones later: on the oracle the best
    # trajectory is then another one than on the context's map, whose costs rank the same with or without it)
    C1 = np.zeros_like(cm)
    C1[:, :int((-38.1 + hw) / (2 * hw / cm.shape[1]))] = 1.0
    n, seeds = 3, (51, 52, 53, 54, 53, 54)
    var = [V.variant("proj2d"), V.variant("temperature3")]
    t = _table(n, 6, 505)
    t[:, 4] = t[:, 2]                                   # the plain twin of the DEM-slot episode
    t[:, 3, 0:2] += np.array(V.COLLISION_START, F32) - np.array(B.START, F32)
    t[:, 5] = t[:, 3]                                   # the plain twin of the costmap-slot episode
    eng = _engine()
    try:
        from mppi_amd import _lib
        batch = _lib.Batch(eng, 6)
        batch.set_variants(var)
        batch.set_dem(0, Z1)
        batch.set_costmap(0, C1)
        for e, (v, d, c) in enumerate([(0, -1, -1), (1, -1, -1), (-1, 0, -1), (-1, -1, 0), (-1, -1, -1), (-1, -1, -1)]):
            batch.set_episode(e, _as_given(t[0, e]), seeds[e], variant=v, dem=d, costmap=c)
        cmds, plans = [], []
        for i in range(n):
            cmd, plan = _step(torch, batch, t[i])
            cmds.append(cmd)
            plans.append(plan)
        cmds, plans = np.array(cmds), np.array(plans)
        refs = [dict(proj="2d", params=V.overridden(var[0])[0]), dict(params=V.overridden(var[1])[0]), dict(Z=Z1),
                dict(cm=C1), dict(), dict()]
        for e, kw in enumerate(refs):
            want, nominal = ref_b(t[:, e], seeds[e], **kw)
            _same_step(cmds[:, e], plans[:, e], want, f"episode {e}")
            _same_nominal(batch, e, nominal, f"episode {e}")
        # the slots act: the twins on the context's scene, same seed and states, plan otherwise
        assert not np.array_equal(_bits(plans[:, 2]), _bits(plans[:, 4]))
        assert not np.array_equal(_bits(plans[:, 3]), _bits(plans[:, 5]))
        batch.close()
    finally:
        eng.close()


# ---- 6. neighbours ----
def _loop(eng, st, first, n, rows):
    """batch_refs.engine_loop's body on a live engine: n closed-loop steps from step index `first`."""
    from mppi_amd import _lib
    r = float(eng.params.robot_radius)
    for i in range(first, first + n):
        assert B.active(st, B.RUN)
        eng.set_state(_lib.make_state(st["x"], st["y"], st["heading"], st["wl"], st["wr"], st["gx"], st["gy"], st["s1"],
                                      st["s2"]))
        o = eng.step("3d", i)
        st, row = B.rule(st, o["traj_sim"][0], o["heading_sim"][0], o["lin_vel"][0], o["ang_vel"][0], r, B.RUN)
        rows.append(row)
    return st


def test_device_step_between_two_runs():
    """run, step_device, run: the second run continues from the ingested state, the step index and the
    nominal sequence the device step left, as the engine-stepped loop does; a batch that never calls
    step_device is the loop of tests/test_gpu_batch.py as before."""
    torch = _gpu()
    from mppi_amd import _lib
    seeds = (61, 62)
    t = _table(1, 2, 606)[0]
    starts = [B.start_state(B.START, FAR), B.start_state((-58.0, -4.0), FAR, (0.0, 1.0, 0.0))]
    pol = _lib.make_policy(**B.RUN)
    eng = _engine()
    try:
        batch = _lib.Batch(eng, 2)
        plain = _lib.Batch(eng, 2)
        for e in range(2):
            batch.set_episode(e, V.mppi_state(starts[e]), seeds[e])
            plain.set_episode(e, V.mppi_state(starts[e]), seeds[e])
        batch.run(3, "3d", pol)
        first = [batch.log(e) for e in range(2)]
        cmd, plan = _step(torch, batch, t)
        batch.run(3, "3d", pol)
        plain.run(6, "3d", pol)
        for e in range(2):
            ref = _engine(seed=seeds[e])
            try:
                rows = []
                _loop(ref, dict(starts[e]), 0, 3, rows)
                assert np.array_equal(_bits(first[e]), _bits(np.array(rows)))
                ref.set_state(_as_given(t[e]))
                want = _plan_of(ref.step("3d", 3))
                _same_step(cmd[e], plan[e], want, f"the device step of episode {e}")
                ingested = dict(x=t[e, 0], y=t[e, 1], heading=t[e, 2:5].astype(np.float64), wl=t[e, 5], wr=t[e, 6],
                                gx=t[e, 7], gy=t[e, 8], s1=t[e, 9], s2=t[e, 10])
                rows = []
                st = _loop(ref, ingested, 4, 3, rows)
                u1, u2 = ref.get_nominal()
            finally:
                ref.close()
            got = V.collect(batch, e)
            assert got["steps"] == 3 and got["total"] == 7 and not got["reached"]
            V.same(got, B._result(rows, st, u1, u2, 3, B.RUN), f"second run of episode {e}")
            V.same(V.collect(plain, e), B.engine_loop(256, H, *_scene(), dict(starts[e]), seeds[e], 6),
                   f"episode {e} of the batch without a device step")
        batch.close()
        plain.close()
    finally:
        eng.close()


def _scene():
    from helpers import c3_scene
    return c3_scene()


# ---- 7. refusals ----
def test_refusals_name_their_cause():
    torch = _gpu()
    from mppi_amd import _lib
    t = _table(1, 2, 707)[0]
    states = _dev(torch, t)

    def refused(batch, code, *words, io=None):
        if io is None:
            io = _lib.MppiBatchIo()
            io.states = states.data_ptr()
        rc = batch.lib.mppi_batch_step_device(batch.h, 3, C.byref(io) if io else None)
        msg = batch.lib.mppi_last_error().decode()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    bare = _lib.Engine(_lib.make_params(256, H), 0)
    try:
        batch = _lib.Batch(bare, 2)
        refused(batch, MPPI_ESTATE, "no DEM")
        with pytest.raises(RuntimeError, match="no DEM"):
            batch.step_device(states)
        batch.close()
    finally:
        bare.close()
    eng = _engine()
    try:
        batch = _open(eng, t, (71, 72))
        refused(batch, MPPI_EINVAL, "null io", io=False)
        refused(batch, MPPI_EINVAL, "null states", io=_lib.MppiBatchIo())
        # a stale slot geometry
        Z, hw, cm = _scene()
        batch.set_dem(4, Z)
        batch.set_episode(1, _as_given(t[1]), 72, dem=4)
        eng.set_dem(np.zeros((200, 200), F32), hw)
        refused(batch, MPPI_ESTATE, "DEM slot 4", "another geometry")
        eng.set_dem(Z, hw)
        # an unfinished campaign
        far = _lib.make_state(B.START[0], B.START[1], goal_x=FAR[0], goal_y=FAR[1])
        batch.set_tasks([_lib.make_task(far, 80 + i, 4) for i in range(3)])
        done, _ = batch.run_tasks(1, "3d", _lib.make_policy(**B.RUN))
        assert done == 0
        refused(batch, MPPI_ESTATE, "batch_step_device", "campaign is unfinished")
        batch.set_tasks([])
        # the batch is whole after the refused calls: the campaign un-set its episodes, set again they step
        cmd, plan = _sentinels(torch, 2)
        got, _ = _step(torch, batch, t, cmd=cmd, plan=plan)
        assert (got == SENTINEL).all()
        batch.set_episode(0, _as_given(t[0]), 71)
        got, got_plan = _step(torch, batch, t, cmd=cmd, plan=plan)
        want, _ = ref_b(t[0:1], 71)
        _same_step(got[0], got_plan[0], want[0], "episode 0 after the refusals")
        assert (got[1] == SENTINEL).all() and (got_plan[1] == SENTINEL).all()
        batch.close()
    finally:
        eng.close()
