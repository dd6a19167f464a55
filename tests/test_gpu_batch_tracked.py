"""GPU: tracked device steps (include/mppi.h mppi_batch_set_tracking / _step_tracked / _get_runs,
DESIGN.md §3.7): the device step with the notion of a run.

A run is logged, tested against its goal and step cap, scored and ended by the ingest kernel, with no
host copy in between.  Checked here: the log rows, results and score rows against Batch.run and the log
scorers, bit for bit; that every step that is taken is still the plain device step's; `done`, ended
episodes and resets; and that tracking off leaves nothing behind.  Helpers, scene and shapes are those
of tests/test_gpu_batch_step_device.py (H = 20, K = 256 unless stated).
"""
import ctypes as C

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V
import test_gpu_batch_step_device as S

pytestmark = pytest.mark.gpu

F32 = np.float32
H, NP, FAR, SENTINEL = S.H, S.NP, S.FAR, S.SENTINEL
MPPI_EINVAL, MPPI_ESTATE = -1, -3
TOL = B.RUN["goal_tol"]
_bits = S._bits


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _step(torch, batch, rows, z=None, **kw):
    """One tracked step_device from a host table, then the wait for the engine's stream: (cmd, plan,
    done) as ndarrays."""
    cmd, plan, done = batch.step_device(S._dev(torch, rows), z=None if z is None else S._dev(torch, np.asarray(z, F32)),
                                        **kw)
    batch.engine.sync()
    return cmd.cpu().numpy(), plan.cpu().numpy(), done.cpu().numpy()


def _origin(row):
    return V.origin_state(row[0], row[1], row[7], row[8])


def _row(state_row, z, cmd):
    """The log row an ingested state makes beside the command before it."""
    return np.array([state_row[0], state_row[1], z, state_row[2], state_row[3], state_row[4], cmd[0], cmd[1]], F32)


def _same_score(run, i, want, tag):
    """Row i of a runs() dict against one path's score (cost, terms, collisions), bitwise."""
    assert _bits(run["cost"][i]) == _bits(F32(want["cost"])), (tag, run["cost"][i], want["cost"])
    assert np.array_equal(_bits(run["terms"][i]), _bits(np.asarray(want["terms"], F32))), (tag, run["terms"][i],
                                                                                          want["terms"])
    assert run["collisions"][i] == want["collisions"], tag


def _smooth_z(torch, states):
    """An arbitrary smooth pose height of (x, y), in tensor operations."""
    return (0.3 * torch.sin(0.1 * states[:, 0]) + 0.05 * states[:, 1]).contiguous()


# ---- 1. the controller's own model as the plant reproduces Batch.run ----
def test_own_model_reproduces_batch_run():
    """batch_refs.MAIN (one start inside the tolerance, one run to the cap of 10) with advance_state on the
    host as the plant and z = row 0 of plan: `done` decides which plant advances.  After 11 calls the
    log, the results and the score rows are those of a twin batch's Batch.run, bit for bit."""
    torch = S._gpu()
    from mppi_amd import _lib
    from mppi_amd.batch import advance_state, from_mppi_state, pack_states, path_length, state_dict
    n, E = 10, len(B.MAIN)
    starts = [state_dict(s[0], s[1], (1.0, 0.0, 0.0), 0.0, 0.0, g[0], g[1]) for s, g, _, _ in B.MAIN]
    seeds = [m[2] for m in B.MAIN]
    ks = [m[3] for m in B.MAIN]
    yardstick = V.variant("weights")
    eng = S._engine(512)
    try:
        radius = float(eng.params.robot_radius)
        run = S._open(eng, pack_states(starts), seeds, trajectories=ks)
        run.run(n, "3d", _lib.make_policy(**B.RUN))
        dev = S._open(eng, pack_states(starts), seeds, trajectories=ks)
        dev.set_tracking(yardstick, max_steps=n, runs_per_episode=1, keep_log=True, goal_tol=TOL)
        states, z = list(starts), np.zeros(E, F32)
        for _ in range(n + 1):
            cmd, plan, done = _step(torch, dev, pack_states(states), z=z)
            for e in np.nonzero(done == 0)[0]:
                states[e], _ = advance_state(states[e], plan[e, 4 * H:4 * H + 3], plan[e, 4 * H + 3:4 * H + 6],
                                             cmd[e, 0], cmd[e, 1], radius, B.RUN)
                z[e] = plan[e, 4 * H + 2]
        assert (done != 0).all() and done[3] == 1 and done[4] == 2
        assert list(dev.run_counts()) == [1] * E
        want_score = run.score(yardstick)
        got = dev.runs()
        assert list(got["episode"]) == list(range(E))
        for e in range(E):
            info = run.episode(e)
            log = run.log(e)
            assert np.array_equal(_bits(dev.log(e)), _bits(log)), f"log rows of {e}"
            assert got["steps"][e] == info["steps_last_run"] == len(log)
            assert bool(got["reached"][e]) == info["reached"]
            assert got["status"][e] == (1 if info["reached"] else 2)
            assert np.array_equal(_bits(got["state"][e]), _bits(pack_states([from_mppi_state(info["state"])])[0])), e
            _same_score(got, e, dict(cost=want_score["cost"][e], terms=want_score["terms"][e],
                                     collisions=want_score["collisions"][e]), f"episode {e}")
            assert got["rows"][e] == want_score["rows"][e] == len(log)
            assert _bits64(got["length"][e]) == _bits64(path_length(log)), (e, got["length"][e])
            assert dev.episode(e)["reached"] == info["reached"]
        assert got["steps"][3] == 0 and got["steps"][4] == n and got["cost"][3] == 0 and got["cost"][4] != 0
        assert got["length"][4] > 0
        # the log scorer answers for the tracked log as for the twin's
        again = dev.score(yardstick)
        for k in ("cost", "terms"):
            assert np.array_equal(_bits(again[k]), _bits(want_score[k])), k
        run.close()
        dev.close()
    finally:
        eng.close()


# ---- 2. a plant that is not the model, without synchronisation ----
def test_plant_on_the_device_without_host_synchronisation():
    """E = 3, the torch unicycle on a non-default stream, 12 calls with a cap of 11 rows and one
    synchronize at the end: the logged rows are the ingested poses beside the commands before them, the
    score rows are mppi_score_paths' of those rows, and the recorded states replayed through reference B
    give the same cmd and plan as the plain device step."""
    torch = S._gpu()
    E, n, seeds = 3, 12, (31, 32, 33)
    start = S._table(1, E, 77)[0]
    stream = torch.cuda.Stream()
    eng = S._engine()
    try:
        eng.set_stream(stream.cuda_stream)
        batch = S._open(eng, start, seeds)
        batch.set_tracking(max_steps=n - 1, keep_log=True, goal_tol=TOL)
        host = torch.as_tensor(start).pin_memory()
        with torch.cuda.stream(stream):
            states = host.to("cuda", non_blocking=True)
            seen = torch.empty((n, E, 11), dtype=torch.float32, device="cuda")
            zs = torch.empty((n, E), dtype=torch.float32, device="cuda")
            cmds = torch.empty((n, E, 2), dtype=torch.float32, device="cuda")
            plans = torch.empty((n, E, NP), dtype=torch.float32, device="cuda")
            dones = torch.empty((n, E), dtype=torch.int32, device="cuda")
            cmd, plan = S._sentinels(torch, E)
            done = torch.zeros(E, dtype=torch.int32, device="cuda")
            for i in range(n):
                seen[i].copy_(states)
                z = _smooth_z(torch, states)
                zs[i].copy_(z)
                batch.step_device(states, cmd=cmd, plan=plan, z=z, done=done)
                cmds[i].copy_(cmd)
                plans[i].copy_(plan)
                dones[i].copy_(done)
                S._unicycle(torch, states, cmd)
        stream.synchronize()
        seen, zs, cmds, plans, dones = (a.cpu().numpy() for a in (seen, zs, cmds, plans, dones))
        assert (dones[:-1] == 0).all() and (dones[-1] == 2).all()
        assert (seen[1:, :, 0:2] != seen[:-1, :, 0:2]).any(axis=-1).all()     # the plant moved every rover
        assert list(batch.run_counts()) == [1] * E
        for e in range(E):
            rows = np.array([_row(seen[i + 1, e], zs[i + 1, e], cmds[i, e]) for i in range(n - 1)], F32)
            assert np.array_equal(_bits(batch.log(e)), _bits(rows)), f"log of {e}"
            run = batch.runs(e)
            assert run["status"][0] == 2 and run["steps"][0] == run["rows"][0] == n - 1 and not run["reached"][0]
            assert np.array_equal(_bits(run["state"][0]), _bits(seen[-1, e]))
            _same_score(run, 0, V.score_one(eng, rows, _origin(seen[0, e])), f"episode {e}")
            assert run["cost"][0] != 0
            # the step itself is untouched by tracking (the 12th call ended the run and took no step)
            want, nominal = S.ref_b(seen[:-1, e], seeds[e])
            S._same_step(cmds[:-1, e], plans[:-1, e], want, f"episode {e}")
            S._same_nominal(batch, e, nominal, f"episode {e}")
            assert np.array_equal(_bits(cmds[-1, e]), _bits(cmds[-2, e]))
        batch.close()
    finally:
        eng.close()


# ---- 3. keep_log = False ----
def test_results_do_not_depend_on_the_log():
    """The same inputs with and without a log: the same results table and counts, bit for bit; without
    one Batch.log answers as a batch without rows does."""
    torch = S._gpu()
    E, n, seeds = 3, 9, (41, 42, 43)
    t = S._table(n, E, 303, near=1)
    resets = {4: [0, 1, 0], 6: [1, 0, 0]}
    eng = S._engine()
    try:
        tables = []
        for keep in (True, False):
            batch = S._open(eng, t[0], seeds)
            batch.set_tracking(max_steps=3, runs_per_episode=3, keep_log=keep, goal_tol=TOL)
            for i in range(n):
                kw = dict(reset=S._dev(torch, resets[i], torch.int32)) if i in resets else {}
                _step(torch, batch, t[i], z=0.01 * t[i, :, 0] - 0.02 * t[i, :, 1], **kw)
            tables.append((batch.runs(), batch.run_counts()))
            if not keep:
                for e in range(E):
                    assert batch.log(e).shape == (0, 8) and batch.episode(e)["steps_last_run"] == 0
                row = np.zeros(8, F32)
                rc = batch.lib.mppi_batch_get_log(batch.h, 0, 0, 1, row.ctypes.data_as(C.POINTER(C.c_float)))
                assert rc == MPPI_EINVAL and b"beyond the steps" in batch.lib.mppi_last_error()
            batch.close()
        (a, ca), (b, cb) = tables
        assert list(ca) == list(cb) and sum(ca) >= 4 and set(a) == set(b)
        assert (a["status"] != 0).sum() >= 4 and a["cost"].any()
        for k in a:
            same = _bits64(a[k]) == _bits64(b[k]) if a[k].dtype == np.float64 else (
                _bits(a[k]) == _bits(b[k]) if a[k].dtype == F32 else a[k] == b[k])
            assert np.all(same), k
    finally:
        eng.close()


# ---- 4. z = None: the episode's DEM ----
def test_z_from_the_dem_is_the_rollouts_lookup():
    """Without z the logged height is oracle.mppi_ref.bilinear(get_corners_heights(...)) at the ingested
    (x, y), bitwise: one episode on the context's DEM and one on a DEM slot of the batch, with states at
    negative and positive x and y (the truncating fraction changes sign with them)."""
    torch = S._gpu()
    from helpers import c3_scene
    from oracle import mppi_ref as R
    Z, hw, cm = c3_scene()
    Z1 = np.ascontiguousarray(Z[::-1, ::-1])
    n, E, seeds = 5, 2, (51, 52)
    t = S._table(n, E, 404)
    spots = [(-60.0, -5.0), (10.3, 12.7), (-41.27, 33.1), (22.9, -17.45), (-0.013, -0.021)]
    for i, (x, y) in enumerate(spots):
        t[i, :, 0] += F32(x) - F32(B.START[0])
        t[i, :, 1] += F32(y) - F32(B.START[1])
    assert (t[1:, :, 0] < 0).any() and (t[1:, :, 0] > 0).any() and (t[1:, :, 1] < 0).any() and (t[1:, :, 1] > 0).any()
    eng = S._engine()
    try:
        from mppi_amd import _lib
        batch = _lib.Batch(eng, E)
        batch.set_dem(0, Z1)
        batch.set_episode(0, S._as_given(t[0, 0]), seeds[0])
        batch.set_episode(1, S._as_given(t[0, 1]), seeds[1], dem=0)
        batch.set_tracking(max_steps=n, keep_log=True, goal_tol=TOL)
        cmds = [_step(torch, batch, t[i])[0] for i in range(n)]
        for e, dem in enumerate((Z, Z1)):
            sc = R.Scene(dem, hw, cm)
            log = batch.log(e)
            assert log.shape == (n - 1, 8)
            for i in range(1, n):
                x, y = t[i, e, 0:1].copy(), t[i, e, 1:2].copy()
                want = R.bilinear(x, y, R.get_corners_heights(sc, x, y), sc.res)
                assert _bits(log[i - 1, 2]) == _bits(F32(want[0])), (e, i, log[i - 1, 2], want)
                assert np.array_equal(_bits(log[i - 1]), _bits(_row(t[i, e], F32(want[0]), cmds[i - 1][e]))), (e, i)
            assert np.abs(log[:, 2]).max() > 0
        # the slot acts: the two DEMs differ where the rovers are
        assert not np.array_equal(batch.log(0)[:, 2], batch.log(1)[:, 2])
        batch.close()
    finally:
        eng.close()


# ---- 5. done, ended episodes and resets ----
def test_done_ended_episodes_and_resets():
    """An episode put inside the tolerance reads done = 1 and one at the cap 2: their sentinel rows, nominal
    sequence and step index stay; a reset starts the next run as a fresh episode with the new seed; a reset of
    an unfinished run with rows records it as abandoned; three runs into two result rows leave a count of 3.
    (A cap of 3 rows, 7 calls; the calls' resets are in `calls`.)"""
    torch = S._gpu()
    E, seeds, NEW = 4, (61, 62, 63, 64), 77
    t = S._table(7, E, 505)
    inside = lambda row: (row[7] - F32(0.2), row[8] + F32(0.1))      # noqa: E731
    t[1, 0, 0:2] = inside(t[1, 0])
    t[5, 0, 0:2] = inside(t[5, 0])
    t[6, 0, 0:2] = inside(t[6, 0])
    zs = (0.02 * t[:, :, 0] + 0.01 * t[:, :, 1]).astype(F32)
    i32, i64 = torch.int32, torch.int64
    calls = [dict(), dict(),
             dict(reset=S._dev(torch, [0, 1, 0, 0], i32), seeds=S._dev(torch, [0, NEW, 0, 0], i64)),
             dict(),
             dict(reset=S._dev(torch, [1, 0, 1, 0], i32)),
             dict(),
             dict(reset=S._dev(torch, [1, 0, 0, 0], i32))]
    eng = S._engine()
    try:
        batch = S._open(eng, t[0], seeds)
        batch.set_tracking(max_steps=3, runs_per_episode=2, keep_log=True, goal_tol=TOL)
        cmds, plans, dones, infos = [], [], [], []
        for i, kw in enumerate(calls):
            cmd, plan = S._sentinels(torch, E)
            cmd, plan, done = _step(torch, batch, t[i], z=zs[i], cmd=cmd, plan=plan, **kw)
            cmds.append(cmd)
            plans.append(plan)
            dones.append(done)
            infos.append([batch.episode(e) for e in range(E)])
        cmds, plans, dones = np.array(cmds), np.array(plans), np.array(dones)
        # (episode 1's second run: start at call 2, rows at calls 3, 4, 5: the cap)
        assert dones.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 2, 2], [0, 0, 0, 2], [1, 2, 0, 2],
                                  [1, 2, 0, 2]]
        # an ended episode took no step: sentinel rows, and (unless the call reset it) its nominal sequence
        # and step index as they were
        for i, e in [(1, 0), (2, 0), (3, 0), (3, 2), (3, 3), (4, 3), (5, 0), (5, 1), (5, 3), (6, 0), (6, 1), (6, 3)]:
            assert (cmds[i, e] == SENTINEL).all() and (plans[i, e] == SENTINEL).all(), (i, e)
            if (i, e) == (6, 0):      # reset into a start inside the tolerance: a fresh episode that took no step
                assert infos[i][e]["steps_total"] == 0 and not infos[i][e]["u1"].any()
                continue
            assert infos[i][e]["steps_total"] == infos[i - 1][e]["steps_total"], (i, e)
            assert np.array_equal(_bits(infos[i][e]["u1"]), _bits(infos[i - 1][e]["u1"])), (i, e)
            assert np.array_equal(_bits(infos[i][e]["u2"]), _bits(infos[i - 1][e]["u2"])), (i, e)
        assert infos[1][0]["reached"] and infos[3][2]["steps_total"] == 3 and not infos[3][2]["reached"]
        # every step that was taken is the plain device step's: episode 1 around its reset, episode 2 to its cap
        want, _ = S.ref_b(t[[0, 1], 1], seeds[1])
        S._same_step(cmds[[0, 1], 1], plans[[0, 1], 1], want, "episode 1, run 0")
        want, nominal = S.ref_b(t[[2, 3, 4], 1], NEW)
        S._same_step(cmds[2:5, 1], plans[2:5, 1], want, "episode 1, run 1: a fresh episode with the new seed")
        S._same_nominal(batch, 1, nominal, "episode 1, run 1")
        want, _ = S.ref_b(t[[0, 1, 2], 2], seeds[2])
        S._same_step(cmds[[0, 1, 2], 2], plans[[0, 1, 2], 2], want, "episode 2, run 0")
        want, _ = S.ref_b(t[[4], 0], seeds[0])
        S._same_step(cmds[[4], 0], plans[[4], 0], want, "episode 0, run 1: its own seed from step 0")
        # the results
        assert list(batch.run_counts()) == [3, 2, 1, 1]
        r = [batch.runs(e) for e in range(E)]
        assert r[0]["status"].tolist() == [1, 1] and r[0]["steps"].tolist() == [1, 1] and r[0]["reached"].tolist() == [1, 1]
        assert np.array_equal(_bits(r[0]["state"]), _bits(t[[1, 5], 0]))
        assert r[1]["status"].tolist() == [3, 2] and r[1]["steps"].tolist() == [1, 3] and not r[1]["reached"].any()
        assert np.array_equal(_bits(r[1]["state"]), _bits(t[[1, 5], 1]))      # abandoned: its last ingested state
        for e in (2, 3):
            assert r[e]["status"].tolist() == [2, 0] and r[e]["steps"].tolist() == [3, 0] and not r[e]["reached"].any()
            assert np.array_equal(_bits(r[e]["state"][0]), _bits(t[3, e]))
        # the score rows: a run of one row, the abandoned one, and the capped ones
        paths = {(0, 0): ([1], 0), (0, 1): ([5], 4), (1, 0): ([1], 0), (1, 1): ([3, 4, 5], 2), (2, 0): ([1, 2, 3], 0),
                 (3, 0): ([1, 2, 3], 0)}
        for (e, k), (ingests, first) in paths.items():
            rows = np.array([_row(t[i, e], zs[i, e], cmds[i - 1, e]) for i in ingests], F32)
            _same_score(r[e], k, V.score_one(eng, rows, _origin(t[first, e])), f"episode {e} run {k}")
            assert r[e]["rows"][k] == len(rows) and r[e]["cost"][k] != 0
        # the log holds the current or most recent run: episode 2's second run so far, the others' ended ones
        assert np.array_equal(_bits(batch.log(1)), _bits(np.array([_row(t[i, 1], zs[i, 1], cmds[i - 1, 1])
                                                                   for i in (3, 4, 5)], F32)))
        assert np.array_equal(_bits(batch.log(2)), _bits(np.array([_row(t[i, 2], zs[i, 2], cmds[i - 1, 2])
                                                                   for i in (5, 6)], F32)))
        assert np.array_equal(_bits(batch.log(3)), _bits(np.array([_row(t[i, 3], zs[i, 3], cmds[i - 1, 3])
                                                                   for i in (1, 2, 3)], F32)))
        batch.close()
    finally:
        eng.close()


# ---- 6. variants and scene slots ----
def test_variants_and_scene_slots_score_on_their_own_costmap():
    """A 2D variant with a body-slope / w_orientation critic row, an episode on its own costmap slot and a
    plain one, under a context whose w_orientation is set: the tracked score rows are Batch.score()'s of
    the logged rows, each on the episode's own costmap."""
    torch = S._gpu()
    from helpers import c3_scene
    from mppi_amd import _lib
    Z, hw, cm = c3_scene()
    C1 = np.zeros_like(cm)
    C1[:, :int((-38.1 + hw) / (2 * hw / cm.shape[1]))] = 1.0       # a wall over x < -38.1
    n, E, seeds = 6, 3, (71, 72, 73)
    var = dict(V.variant("proj2d"), slope="body", w_orientation=0.7)
    t = S._table(n, E, 606)
    t[:, 1, 0:2] += np.array(V.COLLISION_START, F32) - np.array(B.START, F32)
    eng = S._engine()
    try:
        eng.set_critics("wheels", 1.5)
        batch = _lib.Batch(eng, E)
        batch.set_variants([var])
        batch.set_costmap(0, C1)
        for e, (v, c) in enumerate([(0, -1), (-1, 0), (-1, -1)]):
            batch.set_episode(e, S._as_given(t[0, e]), seeds[e], variant=v, costmap=c)
        batch.set_tracking(max_steps=n - 1, keep_log=True, goal_tol=TOL)
        cmds = []
        for i in range(n):
            cmd, _, done = _step(torch, batch, t[i])
            cmds.append(cmd)
        assert done.tolist() == [2] * E
        got, want = batch.runs(), batch.score()
        logs = [batch.log(e) for e in range(E)]
        assert list(want["rows"]) == [n - 1] * E == list(got["rows"])
        for k in ("cost", "terms"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, got[k], want[k])
        assert np.array_equal(got["collisions"], want["collisions"])
        for e in range(E):      # the logged commands are the steps' own
            assert np.array_equal(_bits(logs[e][:, 6:8]), _bits(np.array(cmds)[:-1, e]))
        # the slot acts, and only on its episode: the same rows on the context's costmap score otherwise
        ctx = [V.score_one(eng, logs[e], _origin(t[0, e])) for e in range(E)]
        assert got["collisions"][1] > 0 and _bits(got["terms"][1, 3]) != _bits(ctx[1]["terms"][3])
        for e in (0, 2):
            _same_score(got, e, ctx[e], f"episode {e} on the context's costmap")
        batch.close()
    finally:
        eng.close()


# ---- 7. tracking off ----
def test_tracking_off_leaves_the_plain_step():
    """A tracked step is the plain step's bits; after clear_tracking step_device is the call it was (two
    outputs, the bits of a batch that never had tracking) and the tracked entry answers MPPI_ESTATE; while
    tracking is set the own-model run is refused."""
    torch = S._gpu()
    from mppi_amd import _lib
    E, seeds = 2, (81, 82)
    t = S._table(3, E, 707)
    eng = S._engine()
    try:
        plain = S._open(eng, t[0], seeds)
        tracked = S._open(eng, t[0], seeds)
        tracked.set_tracking(max_steps=5, goal_tol=TOL)
        with pytest.raises(RuntimeError, match="tracking is set"):
            tracked.run(1, "3d", _lib.make_policy(**B.RUN))
        want = [S._step(torch, plain, t[i]) for i in range(3)]
        cmd, plan, _ = _step(torch, tracked, t[0])
        S._same_step(cmd, plan, want[0][1], "the tracked step")
        tracked.clear_tracking()
        for i in (1, 2):
            out = tracked.step_device(S._dev(torch, t[i]))
            assert len(out) == 2
            eng.sync()
            S._same_step(out[0].cpu().numpy(), out[1].cpu().numpy(), want[i][1], f"step {i} after clear_tracking")
        for e in range(E):
            a, b = tracked.episode(e), plain.episode(e)
            assert a["steps_total"] == b["steps_total"] == 3
            assert np.array_equal(_bits(a["u1"]), _bits(b["u1"])) and np.array_equal(_bits(a["u2"]), _bits(b["u2"]))
        io = _lib.MppiBatchIo()
        io.states = S._dev(torch, t[0]).data_ptr()
        rc = tracked.lib.mppi_batch_step_tracked(tracked.h, 3, C.byref(io), None, None)
        assert rc == MPPI_ESTATE and b"tracking is not set" in tracked.lib.mppi_last_error()
        with pytest.raises(RuntimeError, match="tracking is not set"):
            tracked.runs()
        with pytest.raises(ValueError, match="set_tracking first"):
            tracked.step_device(S._dev(torch, t[0]), z=S._dev(torch, np.zeros(E, F32)))
        plain.close()
        tracked.close()
    finally:
        eng.close()
