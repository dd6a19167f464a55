"""GPU: path scoring (mppi_score_paths) and per-critic terms of a step (mppi_get_cost_terms).

The reference for every value is oracle.mppi_ref.critics: the total as it stands, each critic from the
same function with that critic's weight 1 and the others 0 (with finite terms that is the term itself).
Every comparison is exact equality of float32 values.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import helpers as hp
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
H_ENGINE = 100            # the scoring engine's own H: its horizon (9 m) does not depend on the paths' length
WEIGHTS = ("w_path", "w_slope", "w_speed", "w_obstacle")
ORIGIN = hp.START
GOALS = {"far": (65.0, 10.0), "near": (-55.0, -2.0), "inside2m": (-59.0, -4.5)}
N_MAX, L_MAX = 257, 130


def _params(n, L, **kw):
    return R.Params(K=n, H=L, horizon=0.045 * 2.0 * H_ENGINE, **kw)


def oracle_scores(p, sc, st, traj, lw, rw, v):
    """(cost [n], terms [n, 4], collisions [n]) from oracle.mppi_ref.critics / costmap_at."""
    cost = R.critics(p, sc, st, traj, lw, rw, v)
    terms = np.stack([R.critics(dataclasses.replace(p, **{w: (1.0 if w == one else 0.0) for w in WEIGHTS}),
                                sc, st, traj, lw, rw, v) for one in WEIGHTS], -1)
    col = (R.costmap_at(sc, traj[:, :, 0], traj[:, :, 1]) > p.f("collision_threshold")).sum(1).astype(np.int32)
    return cost, terms, col


def recombine(p, terms):
    """critics_warp.py:325-329 in the kernel's order, float32."""
    cost = p.f("w_path") * terms[:, 0]
    cost = cost + p.f("w_slope") * terms[:, 1]
    cost = cost + p.f("w_speed") * terms[:, 2]
    cost = cost + p.f("w_obstacle") * terms[:, 3]
    return cost.astype(F32)


def check(got, want, what):
    cost, terms, col = want
    assert np.isfinite(terms).all(), f"{what}: the oracle's terms must be finite"
    for name, g, w in (("cost", got["cost"], cost), ("terms", got["terms"], terms),
                       ("collisions", got["collisions"], col)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert np.array_equal(g, w), f"{what}: " + hp.mismatch_report(name, g, w)


@functools.lru_cache(maxsize=1)
def rollouts():
    """N_MAX rollouts of L_MAX steps from random controls on the C3 scene (a prefix of a rollout is the
    rollout of the shorter horizon), then shifted: of every 8 paths one leaves the costmap on each of
    its four sides and one starts on a cell above the collision threshold.  Computed once, read-only."""
    Z, hw, cm = hp.c3_scene()
    sc = R.Scene(Z, hw, cm)
    st = hp.oracle_state(wl=1.0, wr=1.2)
    p = _params(N_MAX, L_MAX)
    rng = np.random.default_rng(7)
    u1 = rng.uniform(-1, 1, (N_MAX, L_MAX)).astype(F32)
    u2 = rng.uniform(-1, 1, (N_MAX, L_MAX)).astype(F32)
    v, w = R.wheel_filter(p, st, u1, u2, p.filter_k, p.filter_a)
    traj, _, lw, rw = R.rollout3d(p, sc, st, v, w)
    assert (v >= 0).all()
    iy, ix = np.argwhere(sc.costmap > p.f("collision_threshold"))[0]   # a cell in collision
    ox = (ix + 0.5) * float(sc.res_c) - hw - ORIGIN[0]
    oy = hw - (iy + 0.5) * float(sc.res_c) - ORIGIN[1]
    shift = np.zeros((N_MAX, 2), F32)
    k = np.arange(N_MAX) % 8
    shift[k == 1] = (160.0, 0.0)
    shift[k == 2] = (-40.0, 0.0)
    shift[k == 3] = (0.0, 100.0)
    shift[k == 4] = (0.0, -100.0)
    shift[k == 5] = (ox, oy)
    out = []
    for a in (traj, lw, rw):
        a = a.copy()
        a[:, :, :2] += shift[:, None, :]
        a.setflags(write=False)
        out.append(a)
    v.setflags(write=False)
    return sc, out[0], out[1], out[2], v


@pytest.fixture(scope="module")
def scorer():
    Z, hw, cm = hp.c3_scene()
    eng = hp.engine_for(256, H_ENGINE, Z, hw, cm, hp.oracle_state())
    yield eng
    eng.close()


def _st(goal):
    return hp.oracle_state(goal=GOALS[goal])


@pytest.mark.parametrize("goal", list(GOALS))
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6, 67, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_score_paths_matches_oracle(scorer, n, L, goal):
    sc, traj, lw, rw, v = rollouts()
    traj, lw, rw, v = (np.ascontiguousarray(a[:n, :L]) for a in (traj, lw, rw, v))
    st = _st(goal)
    p = _params(n, L)
    dist = np.hypot(st.goal_x - st.x, st.goal_y - st.y)
    assert {"far": dist > 9.0, "near": 2.0 <= dist <= 9.0, "inside2m": dist < 2.0}[goal]
    want = oracle_scores(p, sc, st, traj, lw, rw, v)
    if n > 5:
        assert want[2][5] > 0, "path 5 starts on a cell in collision"
        x, y = traj[:n, :, 0], traj[:n, :, 1]
        assert (x > sc.hw).any() and (x < -sc.hw).any() and (y > sc.hw).any() and (y < -sc.hw).any()
    got = scorer.score_paths(traj, v, lw, rw, state=hp.state_for(st))
    check(got, want, f"n={n} L={L} {goal}")
    assert np.array_equal(recombine(p, got["terms"]), got["cost"])
    assert scorer.score_ms() > 0.0


@pytest.mark.parametrize("goal", ["far", "near"])
def test_small_odd_costmap_needs_no_dem(goal):
    """A 37 x 37 costmap over 75 m half width (resolution 150/37), scored by an engine that never got a DEM."""
    from mppi_amd import _lib
    sc3, traj, lw, rw, v = rollouts()
    rng = np.random.default_rng(3)
    cm = rng.uniform(0.0, 1.0, (37, 37)).astype(F32)
    cm[rng.uniform(size=cm.shape) < 0.1] = 0.995
    sc = R.Scene(sc3.Z, sc3.half_width, cm)
    n, L = 65, 67
    traj, lw, rw, v = (np.ascontiguousarray(a[:n, :L]) for a in (traj, lw, rw, v))
    st = _st(goal)
    p = _params(n, L)
    want = oracle_scores(p, sc, st, traj, lw, rw, v)
    assert want[2].sum() > 0
    eng = _lib.Engine(_lib.make_params(256, H_ENGINE), 0)
    try:
        eng.set_costmap(cm, sc3.half_width)
        check(eng.score_paths(traj, v, lw, rw, state=hp.state_for(st)), want, f"37x37 {goal}")
    finally:
        eng.close()


@pytest.mark.parametrize("costmap", ["small", "one_cell"])
def test_dumped_rollouts_of_a_non_square_dem(costmap):
    """The rollouts a step on the 120 x 200 DEM (x_min = -30, y_min = -10) dumps, scored on a 50 x 50
    costmap over +-8 m and on a 1 x 1 costmap: as dumped (from the DEM's lower left corner every waypoint
    is outside the small costmap and clamps to one cell) and moved so that they straddle its border."""
    import test_gpu_param_space as PS
    from mppi_amd import _lib
    c = PS.GEOMETRY["nonsquare_corner"]
    dem, st, p = PS._scene(c.scene), c.oracle_state(), c.oracle_params()
    cm = PS._costmap(50) if costmap == "small" else np.full((1, 1), 0.996, F32)
    sc = hp.scene_for(dem.Z, cm, 30.0, resolution=0.25, x_min=-30.0, y_min=-10.0, cm_half_width=8.0)
    eng = _lib.Engine(_lib.make_params(c.K, c.H, **{"seed": PS.SEED, **dict(c.params)}), 0)
    try:
        hp.bind_scene(eng, dem)
        eng.set_state(hp.state_for(st))
        eng.step("3d", 0, copy=False)
        d = eng.dump()
        part = PS._ref(c)[0]["parts"][0]
        for name in ("traj", "lw", "rw", "v"):
            assert np.array_equal(d[name], part[name]), hp.mismatch_report(f"dump {name}", d[name], part[name])
        eng.set_costmap(cm, 8.0)
        for shift in ((0.0, 0.0), (21.9, 11.9)):
            traj, lw, rw = (a.copy() for a in (d["traj"], d["lw"], d["rw"]))
            for a in (traj, lw, rw):
                a[..., :2] += np.asarray(shift, F32)
            x, y = traj[..., 0], traj[..., 1]
            out = (np.abs(x) >= 8.0) | (np.abs(y) >= 8.0)
            if shift == (0.0, 0.0):
                assert out.all()
            else:
                assert (out.any(1) & ~out.all(1)).mean() > 0.05, "no path crosses the costmap's border"
            want = oracle_scores(p, sc, st, traj, lw, rw, d["v"])
            if costmap == "one_cell":
                assert (want[2] == c.H).all()      # the one cell is above the threshold: every waypoint collides
            check(eng.score_paths(traj, d["v"], lw, rw, state=hp.state_for(st)), want, f"{costmap} {shift}")
    finally:
        eng.close()


@pytest.mark.parametrize("n,L", [(65, 67), (64, 130), (1, 3), (5, 4)])
def test_body_slope_mode(scorer, n, L):
    """Without wheel arrays the slope critic runs on the body path: the oracle with lw = rw = traj."""
    sc, traj, _, _, v = rollouts()
    traj, v = (np.ascontiguousarray(a[:n, :L]) for a in (traj, v))
    st = _st("near")
    want = oracle_scores(_params(n, L), sc, st, traj, traj, traj, v)
    check(scorer.score_paths(traj, v, state=hp.state_for(st)), want, f"body n={n} L={L}")


@pytest.mark.parametrize("goal", ["far", "near"])
@pytest.mark.parametrize("wheels", [True, False])
def test_ragged_lengths(scorer, goal, wheels):
    """stride 130 with lengths 1, 3, 4, 67, 130 mixed: each path equals the oracle on its truncated row;
    the rows past a path's length hold NaN and are never read."""
    sc, traj, lw, rw, v = rollouts()
    n = 70
    lengths = np.array([1, 3, 4, 67, 130] * 14, np.int32)
    arrs = [a[:n].copy() for a in (traj, lw, rw, v)]
    for a in arrs:
        for i, ln in enumerate(lengths):
            a[i, ln:] = np.nan
    traj, lw, rw, v = arrs
    if not wheels:
        lw = rw = None
    st = _st(goal)
    got = scorer.score_paths(traj, v, lw, rw, lengths=lengths, state=hp.state_for(st))
    for ln in np.unique(lengths):
        rows = np.nonzero(lengths == ln)[0]
        t, vv = traj[rows, :ln], v[rows, :ln]
        l_, r_ = (lw[rows, :ln], rw[rows, :ln]) if wheels else (t, t)
        want = oracle_scores(_params(len(rows), int(ln)), sc, st, t, l_, r_, vv)
        check({k: a[rows] for k, a in got.items()}, want, f"length {ln} {goal} wheels={wheels}")


@pytest.mark.parametrize("goal", ["far", "near"])
def test_long_path(scorer, goal):
    """n = 3 paths of 3500 waypoints (the reference's loop cap), through the same chunk loop."""
    sc = rollouts()[0]
    n, L = 3, 3500
    rng = np.random.default_rng(11)
    v = rng.uniform(0.0, 2.0, (n, L)).astype(F32)
    step = rng.normal(0.0, 0.06, (n, L, 3)).astype(F32)
    step[:, :, 2] *= F32(0.1)
    traj = (np.array([ORIGIN[0], ORIGIN[1], 0.0], F32) + np.cumsum(step, 1, dtype=F32)).astype(F32)
    off = rng.normal(0.0, 0.2, (2, n, L, 3)).astype(F32)
    lw, rw = traj + off[0], traj + off[1]
    st = _st(goal)
    want = oracle_scores(_params(n, L), sc, st, traj, lw, rw, v)
    check(scorer.score_paths(traj, v, lw, rw, state=hp.state_for(st)), want, f"long {goal}")


def _same_outputs(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: " + hp.mismatch_report(k, a[k], b[k])


def _injected(K, H):
    rng = np.random.default_rng(5)
    return rng.uniform(-1, 1, (K, H)).astype(F32), rng.uniform(-1, 1, (K, H)).astype(F32)


@pytest.mark.parametrize("H,proj,inject", [(12, "3d", False), (100, "3d", False), (12, "2d", False),
                                           (100, "2d", False), (12, "3d", True)])
def test_last_step_terms(H, proj, inject):
    K = 512
    Z, hw, cm = hp.c3_scene()
    sc = R.Scene(Z, hw, cm)
    st = hp.oracle_state(wl=1.0, wr=1.2)
    p = R.Params(K=K, H=H)
    a = hp.engine_for(K, H, Z, hw, cm, st)
    b = hp.engine_for(K, H, Z, hw, cm, st)   # never scores anything
    try:
        if inject:
            u1, u2 = _injected(K, H)
            _same_outputs(a.step_injected(u1, u2, proj), b.step_injected(u1, u2, proj), "injected step")
        else:
            _same_outputs(a.step(proj, 0), b.step(proj, 0), "step 0")
        terms, col = a.cost_terms()
        assert terms.shape == (K, 4) and col.shape == (K,)
        costs = a.costs()
        assert np.array_equal(recombine(p, terms), costs), hp.mismatch_report("recombined", recombine(p, terms), costs)
        d = a.dump()
        want = oracle_scores(p, sc, st, d["traj"], d["lw"], d["rw"], d["v"])
        check(dict(cost=costs, terms=terms, collisions=col), want, f"H={H} {proj}")
        got = a.score_paths(d["traj"], d["v"], d["lw"], d["rw"])   # origin NULL: the context's state
        check(got, want, f"score_paths of the dump H={H} {proj}")
        _same_outputs(a.step(proj, 1), b.step(proj, 1), "the step after scoring")
        assert np.array_equal(a.costs(), b.costs())
    finally:
        a.close()
        b.close()


def test_group_cost_terms():
    """Two members on device 0 (shards of 256 with k_offset): the terms in global order."""
    from mppi_amd import _lib
    K, H = 512, 12
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state(wl=1.0, wr=1.2)
    p = R.Params(K=K, H=H)
    one = hp.engine_for(K, H, Z, hw, cm, st)   # never scores anything
    g = _lib.Group(_lib.make_params(K, H), [0, 0])
    try:
        g.set_dem(Z, hw)
        g.set_costmap(cm, hw)
        g.set_state(hp.state_for(st))
        assert [g.shard(i) for i in range(2)] == [(0, 256), (256, 256)]
        _same_outputs(g.step("3d", 0), one.step("3d", 0), "step 0")
        terms, col = g.cost_terms()
        assert terms.shape == (K, 4) and col.shape == (K,)
        assert np.array_equal(recombine(p, terms), g.costs())
        d = one.dump()
        want = oracle_scores(p, R.Scene(Z, hw, cm), st, d["traj"], d["lw"], d["rw"], d["v"])
        check(dict(cost=g.costs(), terms=terms, collisions=col), want, "group")
        _same_outputs(g.step("3d", 1), one.step("3d", 1), "the step after scoring")
    finally:
        g.close()
        one.close()


def test_controller_optimal_cost_and_terms():
    import yaml
    from mppi_amd.controller import DEFAULT_CONFIG, MPPI_Controller, Robot, Surface
    K, H = 512, 24
    Z, hw, cm = hp.c3_scene()
    with open(DEFAULT_CONFIG) as f:
        cfg = yaml.safe_load(f)
    cfg["controller"]["number_of_trajectories"] = K
    cfg["controller"]["number_of_iterations"] = H
    robot = Robot(-60.0, -5.0, [1.0, 0.0, 0.0], cfg)
    robot.left_wheel_speed = robot.right_wheel_speed = 1.5
    ctl = MPPI_Controller(Surface.from_arrays(Z, cm, hw), robot, cfg, 65.0, 10.0, 0.0)
    ctl.warp_setup()
    ctl.reset("controller")
    ctl.MPPI_step("3d")
    st = R.State(x=-60.0, y=-5.0, left_wheel_speed=1.5, right_wheel_speed=1.5, goal_x=65.0, goal_y=10.0)
    sc = R.Scene(Z, hw, cm)
    p = R.Params(K=K, H=H, seed=42)
    ref = R.mppi_step(p, sc, st, np.zeros(H, F32), np.zeros(H, F32), 0)
    p1 = dataclasses.replace(p, K=1)
    want = oracle_scores(p1, sc, st, ref["traj_sim"][None], ref["lw_sim"][None], ref["rw_sim"][None],
                         ref["v_opt"][None])
    cost, terms = ctl.optimal_cost()
    assert isinstance(cost, float) and terms.shape == (4,) and terms.dtype == F32
    assert F32(cost) == want[0][0] and np.array_equal(terms, want[1][0]), (cost, terms, want)
    t = ctl.cost_terms_wp.numpy()
    assert t.shape == (K, 4)
    part = ref["parts"][0]
    wantK = oracle_scores(p, sc, st, part["traj"], part["lw"], part["rw"], part["v"])
    check(dict(cost=ctl.costs_wp.numpy(), terms=t, collisions=ctl.collisions_wp.numpy()), wantK, "controller")
    r = ctl.score_paths(part["traj"][:5], part["v"][:5], part["lw"][:5], part["rw"][:5])
    assert np.array_equal(r["cost"], ref["cost"][:5])
    ctl.engine.close()


MPPI_EINVAL, MPPI_ESTATE = -1, -3


def test_errors_leave_the_context_usable():
    """Every refusal happens on the host before any launch; a step afterwards matches the oracle."""
    from mppi_amd import _lib
    K, H = 256, 12
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state()
    lib = _lib.load_library()
    n, L = 4, 6
    traj = np.zeros((n, L, 3), F32)
    v = np.ones((n, L), F32)
    col = np.zeros(n, np.int32)
    cost = np.zeros(n, F32)
    out = _lib.MppiPathScores(_lib._fp(cost), None, col.ctypes.data_as(C.POINTER(C.c_int32)))
    fp, i32 = _lib._fp, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def score(ctx, n_=n, stride=L, lengths=None, traj_=fp(traj), lw=None, rw=None, v_=fp(v), out_=C.byref(out)):
        return lib.mppi_score_paths(ctx, n_, stride, lengths, traj_, lw, rw, v_, None, out_)

    # before a costmap (and before any step): ESTATE
    bare = _lib.Engine(_lib.make_params(K, H), 0)
    try:
        bare.set_state(hp.state_for(st))
        assert score(bare.ctx) == MPPI_ESTATE
        assert lib.mppi_get_cost_terms(bare.ctx, None, None) == MPPI_ESTATE
    finally:
        bare.close()

    eng = hp.engine_for(K, H, Z, hw, cm, st)
    try:
        assert lib.mppi_get_cost_terms(eng.ctx, None, None) == MPPI_ESTATE      # no step to re-run
        assert score(eng.ctx, traj_=None) == MPPI_EINVAL
        assert score(eng.ctx, v_=None) == MPPI_EINVAL
        assert score(eng.ctx, out_=None) == MPPI_EINVAL
        assert score(eng.ctx, n_=-1) == MPPI_EINVAL
        assert score(eng.ctx, stride=0) == MPPI_EINVAL
        assert score(eng.ctx, lw=fp(traj)) == MPPI_EINVAL
        assert score(eng.ctx, rw=fp(traj)) == MPPI_EINVAL
        for bad in ([1, 2, 0, 3], [1, 2, L + 1, 3], [-5, 1, 1, 1]):
            assert score(eng.ctx, lengths=i32(np.array(bad, np.int32))) == MPPI_EINVAL
            assert "lengths" in lib.mppi_last_error().decode()
        assert score(eng.ctx, n_=1 << 20, stride=1 << 11) == MPPI_EINVAL       # n * stride = 2^31
        assert score(eng.ctx, n_=0) == 0                                        # nothing to do is fine
        assert score(eng.ctx) == 0
        with pytest.raises(ValueError):
            eng.score_paths(traj, v, left_wheel=traj)
        out_step = eng.step("3d", 0)
        ref = R.mppi_step(R.Params(K=K, H=H), R.Scene(Z, hw, cm), st, np.zeros(H, F32), np.zeros(H, F32), 0)
        np.testing.assert_array_equal(eng.costs(), ref["cost"])
        np.testing.assert_array_equal(out_step["u1_opt"], ref["u1_opt"])
        np.testing.assert_array_equal(out_step["traj_sim"], ref["traj_sim"])
    finally:
        eng.close()
