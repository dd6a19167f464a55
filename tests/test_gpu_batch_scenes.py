"""GPU: per-episode DEM, costmap and trajectory count of the batched episodes (mppi_batch_set_dem /
_set_costmap / _build_costmap / _set_episode_scene / _set_episode_trajectories).

Contract: every step of an episode that holds a DEM slot, a costmap slot and a K_e is bitwise the
mppi_step of a context with num_trajectories = K_e after mppi_set_dem / mppi_set_costmap of the
slots' contents.  References A and B and the small scene are in tests/batch_scene_refs.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_scene_refs as S
import batch_variant_refs as V

pytestmark = pytest.mark.gpu

MPPI_EINVAL, MPPI_ESTATE = -1, -3
DEM_SLOT, CM_SLOT = 255, 1023     # the last slot of each table


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _policy(check_every=0):
    from mppi_amd import _lib
    return _lib.make_policy(check_every=check_every, **B.RUN)


def ep(dem=-1, cm=-1, k=0, var=-1, goal=S.GOAL, start=S.START, seed=S.SEED):
    return dict(dem=dem, cm=cm, k=k, var=var, goal=goal, start=start, seed=seed)


def _run(episodes, runs, ctx_k=S.K, dems=None, costmaps=None, variants=None, check_every=0, raw=False,
         between=None):
    """episodes: ep(...) dicts; dems / costmaps: {slot: array}; runs: step caps of successive runs;
    between(batch, engine, i): called before run i > 0.  raw: set the episodes through
    mppi_batch_set_episode alone, touching no other entry point.  Returns per episode the result
    after the last run with the log rows of all runs concatenated."""
    _gpu()
    from mppi_amd import _lib
    eng = S.make_engine(ctx_k)
    try:
        batch = _lib.Batch(eng, len(episodes))
        for slot, Z in (dems or {}).items():
            batch.set_dem(slot, Z)
        for slot, cm in (costmaps or {}).items():
            batch.set_costmap(slot, cm)
        if variants:
            batch.set_variants(variants)
        for e, d in enumerate(episodes):
            st = V.mppi_state(B.start_state(d["start"], d["goal"]))
            if raw:
                assert (d["dem"], d["cm"], d["k"], d["var"]) == (-1, -1, 0, -1)
                assert eng.lib.mppi_batch_set_episode(batch.h, e, C.byref(st), d["seed"]) == 0
            else:
                batch.set_episode(e, st, d["seed"], d["var"], d["dem"], d["cm"], d["k"])
        logs = [[] for _ in episodes]
        for i, n in enumerate(runs):
            if i and between:
                between(batch, eng, i)
            batch.run(n, "3d", _policy(check_every))
            for e in range(len(episodes)):
                logs[e].append(batch.log(e))
        out = []
        for e in range(len(episodes)):
            r = V.collect(batch, e)
            r["rows"] = np.concatenate(logs[e])
            r["steps"] = len(r["rows"])
            assert r["total"] == r["steps"], (e, r["total"], r["steps"])
            out.append(r)
        batch.close()
    finally:
        eng.close()
    return out


# ---- 1. main case ----
# (DEM index, costmap index, K, variant) per episode, as the issue's table
MAIN = [(0, 0, 512, False), (1, 0, 512, False), (0, 1, 512, False), (1, 1, 512, False),
        (0, 0, 300, False), (0, 0, 256, False), (1, 1, 200, False), (1, 1, 300, True)]


def _main_episodes(goal=S.GOAL):
    return [ep(DEM_SLOT if di else -1, CM_SLOT if ci else -1, 0 if k == S.K else k, 0 if var else -1, goal=goal)
            for di, ci, k, var in MAIN]


def _main_run(runs=(S.CAP,), check_every=0, goal=S.GOAL):
    return _run(_main_episodes(goal), runs, dems={DEM_SLOT: S.dem(1)}, costmaps={CM_SLOT: S.costmap(1)},
                variants=[S.variant8()], check_every=check_every)


@functools.lru_cache(maxsize=None)
def _main_case():
    return _main_run()


def _main_ref_a(i, goal=S.GOAL):
    di, ci, k, var = MAIN[i]
    return S.ref_a(di, ci, k, goal=goal, with_variant=var)


def test_main_case_inputs_differ():
    """On the oracle every slot and K_e of the main case changes the loop: a kernel that ignores one
    cannot pass by coincidence."""
    base = _main_ref_a(0)
    assert S.first_difference(_main_ref_a(1), base) == 0          # Z1
    assert S.first_difference(_main_ref_a(2), base) == 1          # C1
    for i in (4, 5, 6):                                           # K_e = 300, 256, 200
        assert S.first_difference(_main_ref_a(i), base) == 0, i
    assert S.first_difference(_main_ref_a(3), _main_ref_a(1)) == 4    # (Z1, C1) against (Z1, C0)
    assert S.first_difference(_main_ref_a(3), _main_ref_a(2)) is not None
    assert S.first_difference(_main_ref_a(7), S.ref_a(1, 1, 300)) is not None   # the variant acts too


@pytest.mark.parametrize("i", range(len(MAIN)))
def test_main_case_matches_references(i):
    """One batch of the eight episodes of the issue's table: each is bitwise reference A (oracle loop)
    and reference B (a fresh engine with that DEM, costmap, K and variant)."""
    got = _main_case()[i]
    di, ci, k, var = MAIN[i]
    V.same(got, _main_ref_a(i), f"episode {i + 1} vs A")
    V.same(got, S.ref_b(di, ci, k, with_variant=var), f"episode {i + 1} vs B")


# ---- 2. edge counts ----
def test_edge_counts_k512():
    """K_e = 1 (one lane), 257 (one valid lane in the second block); 512 given explicitly has the
    default's bits."""
    cap = 6
    got = _run([ep(k=1, goal=S.FAR), ep(k=257, goal=S.FAR), ep(k=512, goal=S.FAR), ep(goal=S.FAR)], (cap,))
    for e, k in enumerate((1, 257, 512)):
        V.same(got[e], S.ref_a(0, 0, k, n_steps=cap, goal=S.FAR), f"K_e = {k} vs A")
        V.same(got[e], S.ref_b(0, 0, k, n_steps=cap, goal=S.FAR), f"K_e = {k} vs B")
        assert got[e]["steps"] == cap
    V.same(got[2], got[3], "K_e = 512 vs the default")
    assert V.differ(got[0], got[3]) >= 1 and V.differ(got[1], got[3]) >= 1


def test_edge_counts_k1280():
    """A context of K = 1280 (five leaf records) with K_e = 1000, 500, 350 (4, 2, 2 records) and the
    default, six steps."""
    cap = 6
    ks = (1000, 500, 350, 1280)
    got = _run([ep(k=0 if k == 1280 else k, goal=S.FAR) for k in ks], (cap,), ctx_k=1280)
    for e, k in enumerate(ks):
        V.same(got[e], S.ref_a(0, 0, k, n_steps=cap, goal=S.FAR), f"K_e = {k} of 1280 vs A")
        V.same(got[e], S.ref_b(0, 0, k, n_steps=cap, goal=S.FAR), f"K_e = {k} of 1280 vs B")
    assert len({got[e]["rows"].tobytes() for e in range(4)}) == 4


# ---- 3. termination and split runs ----
def test_termination_facts_on_the_oracle():
    """The near goal is reached before the cap by every episode of the main case (after different
    numbers of steps, some before and some after step 15 and 16), the far goal by none."""
    steps = []
    for i in range(len(MAIN)):
        near, far = _main_ref_a(i, S.NEAR), _main_ref_a(i, S.FAR)
        assert near["reached"] and 0 < near["steps"] < S.CAP, (i, near["steps"])
        assert not far["reached"] and far["steps"] == S.CAP, i
        steps.append(near["steps"])
    assert len(set(steps)) >= 4 and min(steps) < 15 and max(steps) > 16, steps


@pytest.mark.parametrize("check_every", [1, 7, 16])
def test_termination_does_not_depend_on_check_every(check_every):
    got = _main_run(check_every=check_every, goal=S.NEAR)
    for i in range(len(MAIN)):
        V.same(got[i], _main_ref_a(i, S.NEAR), f"episode {i + 1}, check_every {check_every}")
        assert got[i]["reached"]


def test_far_goal_split_runs():
    """15 + 25 steps to a goal nobody reaches = one oracle loop of 40 steps."""
    got = _main_run(runs=(15, 25), goal=S.FAR)
    for i in range(len(MAIN)):
        V.same(got[i], _main_ref_a(i, S.FAR), f"episode {i + 1}, 15 + 25 steps")
        assert got[i]["steps"] == S.CAP and not got[i]["reached"]


def test_near_goal_split_runs():
    got = _main_run(runs=(15, 25), goal=S.NEAR)
    for i in range(len(MAIN)):
        V.same(got[i], _main_ref_a(i, S.NEAR), f"episode {i + 1}, 15 + 25 steps")


# ---- 4. slot replaced between runs ----
def test_slot_replaced_between_runs():
    """Ten steps, the slots' contents replaced (and the context's DEM changed), ten more: the oracle
    loop that switches scene at step 10.  Episode 2 at -1 picks up the context's new DEM."""
    def swap(batch, eng, i):
        batch.set_dem(DEM_SLOT, S.dem(0))
        batch.set_costmap(CM_SLOT, S.costmap(0))
        eng.set_dem(S.dem(1), S.HW)

    got = _run([ep(DEM_SLOT, CM_SLOT, goal=S.FAR), ep(DEM_SLOT, -1, 300, goal=S.FAR), ep(goal=S.FAR)], (10, 10),
               dems={DEM_SLOT: S.dem(1)}, costmaps={CM_SLOT: S.costmap(1)}, between=swap)
    st = B.start_state(S.START, S.FAR)
    want = [S.oracle_segments(512, [((1, 1), 10), ((0, 0), 10)], st, S.SEED),
            S.oracle_segments(300, [((1, 0), 10), ((0, 0), 10)], st, S.SEED),
            S.oracle_segments(512, [((0, 0), 10), ((1, 0), 10)], st, S.SEED)]
    for e in range(3):
        V.same(got[e], want[e], f"episode {e} across the swap")
        assert got[e]["steps"] == 20
    # the swap does act: the loops that never switch differ in the second half
    assert S.first_difference(want[0], S.ref_a(1, 1, 512, n_steps=20, goal=S.FAR)) >= 10
    assert S.first_difference(want[2], S.ref_a(0, 0, 512, n_steps=20, goal=S.FAR)) >= 10


# ---- 5. no leak, no change ----
def test_neighbours_do_not_leak():
    """Episodes without a slot or K_e, between episodes that hold some, have the bits of a batch that
    never called a new entry point."""
    plain = _run([ep(seed=s) for s in (11, 12, 13)], (12,), raw=True)
    mixed = _run([ep(DEM_SLOT, CM_SLOT, 200), ep(seed=11), ep(-1, CM_SLOT), ep(seed=12), ep(k=300), ep(seed=13),
                  ep(DEM_SLOT)], (12,), dems={DEM_SLOT: S.dem(1)}, costmaps={CM_SLOT: S.costmap(1)})
    for j, e in enumerate((1, 3, 5)):
        V.same(mixed[e], plain[j], f"episode {e} beside scene holders")
    V.same(mixed[0], S.ref_a(1, 1, 200, n_steps=12), "holder 0 vs A")
    V.same(mixed[2], S.ref_a(0, 1, 512, n_steps=12), "holder 2 vs A")
    V.same(mixed[4], S.ref_a(0, 0, 300, n_steps=12), "holder 4 vs A")
    V.same(mixed[6], S.ref_a(1, 0, 512, n_steps=12), "holder 6 vs A")


@pytest.mark.parametrize("check_every", [1, 16])
def test_copies_of_the_context_scene_change_nothing(check_every):
    """Every episode on slots that hold copies of the context's DEM and costmap, with K_e = K: the
    plain batch, across a split run."""
    goals = (S.GOAL, S.FAR, (2.0, 0.4))
    plain = _run([ep(goal=g, seed=20 + i) for i, g in enumerate(goals)], (8, 8), check_every=check_every, raw=True)
    held = _run([ep(0, 0, S.K, goal=g, seed=20 + i) for i, g in enumerate(goals)], (8, 8), check_every=check_every,
                dems={0: S.dem(0)}, costmaps={0: S.costmap(0)})
    for e in range(len(goals)):
        V.same(held[e], plain[e], f"episode {e}, check_every {check_every}")
    assert plain[1]["steps"] == 16


# ---- 6. score ----
def test_score_on_each_episodes_costmap():
    """70 episodes (two tiles of the kernel), costmap slots alternating inside each tile: Batch.score()
    is bitwise score_paths of an engine that holds the episode's costmap."""
    _gpu()
    from mppi_amd import _lib
    E, cap = 70, 10
    inside = (1.7, 1.0)                         # the centre of a blob of C0
    cms = [(-1, 0), (CM_SLOT, 1), (7, 0)]       # (slot, costmap index): the context's, C1, a copy of C0
    eng, eng1 = S.make_engine(), S.make_engine(ci=1)
    try:
        batch = _lib.Batch(eng, E)
        batch.set_costmap(CM_SLOT, S.costmap(1))
        batch.set_costmap(7, S.costmap(0))
        starts = [inside if e % 5 == 0 else (1.0 + 0.01 * e, 1.0) for e in range(E)]
        for e in range(E):
            batch.set_episode(e, V.mppi_state(B.start_state(starts[e], S.FAR)), 100 + e, costmap=cms[e % 3][0],
                              trajectories=256)
        batch.run(cap, "3d", _policy())
        logs = [batch.log(e) for e in range(E)]
        got = batch.score()
        origins = [V.origin_state(starts[e][0], starts[e][1], *S.FAR) for e in range(E)]
        hit = 0
        for e in range(E):
            ci = cms[e % 3][1]
            want = V.score_one(eng1 if ci else eng, logs[e], origins[e])
            assert got["rows"][e] == len(logs[e]) == cap, e
            assert np.float32(got["cost"][e]).view(np.uint32) == np.float32(want["cost"]).view(np.uint32), e
            assert np.array_equal(got["terms"][e].view(np.uint32), np.asarray(want["terms"], np.float32).view(np.uint32)), e
            assert got["collisions"][e] == want["collisions"], e
            if ci == 0 and got["collisions"][e] > 0:
                hit += 1
                # the oracle's critics agree: collisions on its own costmap, none with the rocks removed
                assert S.collisions_on(0, logs[e]) == got["collisions"][e]
                assert S.obstacle_term(0, logs[e], starts[e], S.FAR) >= 100000.0
                assert S.collisions_on(1, logs[e]) == 0 and S.obstacle_term(1, logs[e], starts[e], S.FAR) == 0.0
        assert hit >= 1
        # an episode that starts inside the blob but holds C1 collides with nothing
        free = [e for e in range(E) if e % 5 == 0 and cms[e % 3][1] == 1]
        assert free and all(got["collisions"][e] == 0 for e in free)
        batch.close()
    finally:
        eng.close()
        eng1.close()


# ---- 7. built costmap ----
def test_built_costmap_slot():
    """build_costmap into a slot from 64 rocks is CostmapBuilder.build with the same arguments, and an
    episode on it is an engine given that map."""
    _gpu()
    from mppi_amd import _lib
    rng = np.random.RandomState(5)
    rocks = [[rng.uniform(-15.0, 15.0), rng.uniform(-15.0, 15.0), rng.uniform(0.05, 0.4)] for _ in range(63)]
    origin, r_robot, cap = (0.25, -0.5), 0.3, 12
    # one rock whose inflated disc ends 3 cm ahead of the start, towards the goal.  A rock at global
    # (xg, yg) lies at x = yg - y0, y = -(xg - x0) of the costmap's lookup: this one at (1.5, 1.3).
    # (On the oracle, with the restated cv2 calls, the loop on this map leaves the loop on C0 at step 0.)
    rocks.append([-1.05, 1.0, 0.3])
    builder = _lib.CostmapBuilder(0)
    want = builder.build(rocks, origin, S.N, S.HW, r_robot)
    builder.close()
    assert 0.0 < float(want.mean()) and float(want.max()) > 0.99
    eng = S.make_engine()
    try:
        batch = _lib.Batch(eng, 2)
        got = batch.build_costmap(3, rocks, origin, r_robot, copy_out=True)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert batch.build_costmap(4, rocks, origin, r_robot, power=10, metric="exact") is None
        for e in range(2):
            batch.set_episode(e, V.mppi_state(B.start_state(S.START, S.FAR)), S.SEED, costmap=3 if e == 0 else -1)
        batch.run(cap, "3d", _policy())
        on_slot, on_ctx = V.collect(batch, 0), V.collect(batch, 1)
        batch.close()
    finally:
        eng.close()
    V.same(on_slot, S.ref_b(0, 0, S.K, n_steps=cap, goal=S.FAR, cm=want), "episode on the built map vs B")
    V.same(on_ctx, S.ref_a(0, 0, S.K, n_steps=cap, goal=S.FAR), "episode on the context's map vs A")
    assert V.differ(on_slot, on_ctx) >= 1


# ---- 8. argument checks ----
def test_argument_checks():
    """Every refused call returns its code and names the slot, episode or field, and leaves the batch
    as it was: it runs normally afterwards.  (MPPI_EHIP for a failed slot allocation needs the device's
    memory exhausted and is not provoked here.)"""
    _gpu()
    from mppi_amd import _lib
    eng = S.make_engine()
    try:
        lib = eng.lib
        batch = _lib.Batch(eng, 2)
        z1, c1 = np.ascontiguousarray(S.dem(1)), np.ascontiguousarray(S.costmap(1))
        zp, cp = _lib._fp(z1), _lib._fp(c1)

        def refused(rc, *words, code=MPPI_EINVAL):
            assert rc == code, (rc, lib.mppi_last_error())
            msg = lib.mppi_last_error()
            for w in words:
                assert w.encode() in msg, (w, msg)

        # slot index out of range
        refused(lib.mppi_batch_set_dem(batch.h, 256, zp), "DEM slot 256")
        refused(lib.mppi_batch_set_dem(batch.h, -1, zp), "DEM slot -1")
        refused(lib.mppi_batch_set_costmap(batch.h, 1024, cp), "costmap slot 1024")
        refused(lib.mppi_batch_set_dem(batch.h, 256, None), "DEM slot 256")
        obs = np.zeros(3, np.float64)
        refused(lib.mppi_batch_build_costmap(batch.h, 1024, obs.ctypes.data_as(_lib._DP), 1, 0.0, 0.0, 0.3, 20, 0, None),
                "costmap slot 1024")
        refused(lib.mppi_batch_build_costmap(batch.h, 0, obs.ctypes.data_as(_lib._DP), 1, 0.0, 0.0, 0.3, 20, 9, None),
                "metric")
        # an episode given an empty slot, or one out of range; an episode out of range
        for e in range(2):
            batch.set_episode(e, V.mppi_state(B.start_state(S.START, S.GOAL)), S.SEED)
        refused(lib.mppi_batch_set_episode_scene(batch.h, 0, 5, -1), "episode 0", "DEM slot 5", "empty")
        refused(lib.mppi_batch_set_episode_scene(batch.h, 1, -1, 9), "episode 1", "costmap slot 9", "empty")
        refused(lib.mppi_batch_set_episode_scene(batch.h, 0, 256, -1), "episode 0", "DEM slot 256")
        refused(lib.mppi_batch_set_episode_scene(batch.h, 0, -1, -2), "episode 0", "costmap slot -2")
        refused(lib.mppi_batch_set_episode_scene(batch.h, 2, -1, -1), "episode")
        refused(lib.mppi_batch_set_episode_trajectories(batch.h, 2, 0), "episode")
        # K_e outside [1, context K]
        for k in (513, -1, 1 << 40):
            refused(lib.mppi_batch_set_episode_trajectories(batch.h, 1, k), "episode 1", "num_trajectories")
        # freeing a slot an episode holds
        assert lib.mppi_batch_set_dem(batch.h, DEM_SLOT, zp) == 0
        assert lib.mppi_batch_set_costmap(batch.h, CM_SLOT, cp) == 0
        assert lib.mppi_batch_set_episode_scene(batch.h, 0, DEM_SLOT, CM_SLOT) == 0
        assert lib.mppi_batch_set_episode_trajectories(batch.h, 0, 200) == 0
        refused(lib.mppi_batch_set_dem(batch.h, DEM_SLOT, None), f"DEM slot {DEM_SLOT}", "episode 0")
        refused(lib.mppi_batch_set_costmap(batch.h, CM_SLOT, None), f"costmap slot {CM_SLOT}", "episode 0")
        assert lib.mppi_batch_set_dem(batch.h, 9, None) == 0          # freeing an empty slot is no error
        # the context's geometry changed under a held slot: MPPI_ESTATE from run and score, naming the slot
        small = np.zeros((200, 200), np.float32)
        eng.set_dem(small, S.HW)
        refused(lib.mppi_batch_run(batch.h, 3, 1, C.byref(_policy())), f"DEM slot {DEM_SLOT}", code=MPPI_ESTATE)
        eng.set_dem(S.dem(0), S.HW)
        eng.set_costmap(small, S.HW)
        refused(lib.mppi_batch_run(batch.h, 3, 1, C.byref(_policy())), f"costmap slot {CM_SLOT}", code=MPPI_ESTATE)
        sc = _lib.MppiPathScores()
        refused(lib.mppi_batch_score(batch.h, None, None, C.byref(sc), None), f"costmap slot {CM_SLOT}",
                code=MPPI_ESTATE)
        # a slot set under that geometry cannot take the old size's array through the wrapper
        with pytest.raises(ValueError):
            batch.set_costmap(0, c1)
        eng.set_costmap(S.costmap(0), S.HW)
        # the scene and K_e outlive set_episode, and the batch is as before the refused calls
        batch.set_episode(1, V.mppi_state(B.start_state(S.START, S.GOAL)), S.SEED)
        assert lib.mppi_batch_set_episode(batch.h, 0, C.byref(V.mppi_state(B.start_state(S.START, S.GOAL))), S.SEED) == 0
        batch.run(S.CAP, "3d", _policy())
        V.same(V.collect(batch, 0), S.ref_a(1, 1, 200), "episode 0 after the refused calls")
        V.same(V.collect(batch, 1), S.ref_a(0, 0, 512), "episode 1 after the refused calls")
        # released, the slots can be freed; an episode cannot take them any more
        assert lib.mppi_batch_set_episode_scene(batch.h, 0, -1, -1) == 0
        assert lib.mppi_batch_set_dem(batch.h, DEM_SLOT, None) == 0
        assert lib.mppi_batch_set_costmap(batch.h, CM_SLOT, None) == 0
        refused(lib.mppi_batch_set_episode_scene(batch.h, 0, DEM_SLOT, -1), "empty")
        batch.close()
    finally:
        eng.close()


def test_slots_need_the_context_scene_first():
    """A slot takes the context's geometry: MPPI_ESTATE before the context has a DEM / costmap."""
    _gpu()
    from mppi_amd import _lib
    eng = _lib.Engine(_lib.make_params(S.K, S.H), 0)
    try:
        batch = _lib.Batch(eng, 1)
        z = np.zeros((S.N, S.N), np.float32)
        assert eng.lib.mppi_batch_set_dem(batch.h, 0, _lib._fp(z)) == MPPI_ESTATE
        assert eng.lib.mppi_batch_set_costmap(batch.h, 0, _lib._fp(z)) == MPPI_ESTATE
        with pytest.raises(RuntimeError):
            batch.set_dem(0, z)
        batch.close()
    finally:
        eng.close()


# ---- MPPI_Controller.run_batch ----
def test_run_batch_scenes():
    """run_batch with dems / costmaps (an array and a rock list) / episode_trajectories: the trails are
    those of the oracle loop on each episode's scene and K_e, and of an engine on the built rock map."""
    _gpu()
    from mppi_amd import _lib, controller
    cap = 8
    cfg = controller._load_config(controller.DEFAULT_CONFIG)
    cfg = {**cfg, "controller": {**cfg["controller"], "number_of_trajectories": S.K, "number_of_iterations": S.H},
           "engine": {**(cfg.get("engine") or {}), "seed": S.SEED}}
    surface = controller.Surface.from_arrays(S.dem(0), S.costmap(0), S.HW, radius_robot=0.3)
    robot = controller.Robot(S.START[0], S.START[1], [1.0, 0.0, 0.0], cfg)
    ctl = controller.MPPI_Controller(surface, robot, cfg, S.FAR[0], S.FAR[1], 0.0)
    ctl.std_dev_u1 = ctl.std_dev_u2 = 0.25
    rocks = [[-1.05, 1.0, 0.3], [6.0, -3.0, 0.2]]
    origin = (0.25, -0.5)
    res = ctl.run_batch([S.START] * 4, [(1.0, 0.0, 0.0)] * 4, [S.FAR] * 4, seeds=[S.SEED] * 4, max_loops=cap,
                        dems=[S.dem(1)], costmaps=[S.costmap(1).ravel(), dict(obstacles=rocks, origin=origin)],
                        episode_dem=[None, 0, -1, -1], episode_costmap=[-1, 0, 1, None],
                        episode_trajectories=[0, 300, None, 200])
    ctl.engine.close()
    builder = _lib.CostmapBuilder(0)
    built = builder.build(rocks, origin, S.N, S.HW, 0.3)
    builder.close()
    want = [S.ref_a(0, 0, S.K, n_steps=cap, goal=S.FAR), S.ref_a(1, 1, 300, n_steps=cap, goal=S.FAR),
            S.ref_b(0, 0, S.K, n_steps=cap, goal=S.FAR, cm=built), S.ref_a(0, 0, 200, n_steps=cap, goal=S.FAR)]
    assert len(res) == 4
    for e, (r, w) in enumerate(zip(res, want)):
        assert r["loops"] == cap and not r["reached"], e
        for key, col in (("x", 0), ("y", 1), ("z", 2)):
            got = np.asarray(r[key][1:], np.float32)
            assert np.array_equal(got.view(np.uint32), w["rows"][:, col].view(np.uint32)), (e, key)
        assert np.array_equal(np.asarray(r["lin_vel"], np.float32).view(np.uint32), w["rows"][:, 6].view(np.uint32)), e
    assert S.first_difference(want[2], want[0]) is not None     # the rock list acts
