"""GPU: steps off the default parameters and off the square, centred grid, against the oracle bit for bit.

Every other parity test runs the C3 scene with make_params' defaults.  Here the numbers a caller of
the C-ABI changes first vary instead: the angular bound around RolloutArgs::small_angle's 0.78
threshold (the range-reduced sin / cos arm), reverse driving, asymmetric control limits, the wheel
offset and radius, dt and the horizon, the collision rule, the filters' edges a = 0 and a = 1,
sigma 0, headings in every quadrant; and the grid: rows != cols, x_min != -y_min, resolutions 0.1,
0.07 and 1/3, costmaps coarser than, as fine as and smaller than the DEM, a 1 x 1 costmap, a 2 x 2
DEM, a robot wholly outside the map, and the IEEE cell division (mppi_set_option
"verified_reciprocal" 0).  Each case runs on the role-split kernel, the pair kernel and (3D) the
resident server, and compares every output of every step, the costs, the dumped rollouts and the
per-critic terms with np.array_equal.

Every case first asserts, on the oracle's own arrays, that it exercises what it is named for, and
that the oracle's costs and outputs are finite.  The oracle of a case is computed once and shared
by the modes.  Shapes: K <= 300, H <= 24, DEMs <= 285^2.
"""
import dataclasses
import functools

import numpy as np
import pytest

import helpers as hp
from mppi_amd import scene
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
OUTS = (("u1_opt", "u1_opt"), ("u2_opt", "u2_opt"), ("lin_vel", "v_opt"), ("ang_vel", "w_opt"),
        ("traj_sim", "traj_sim"), ("heading_sim", "hv_sim"), ("left_wheel_sim", "lw_sim"),
        ("right_wheel_sim", "rw_sim"))
DUMPS = ("traj", "hv", "lw", "rw", "v", "w", "u1", "u2")
WEIGHTS = ("w_path", "w_slope", "w_speed", "w_obstacle")
MODES = ("roles", "pair", "server")
MODES_2D = ("roles", "pair")
START, GOAL = (-12.0, -3.0), (15.0, 5.0)
K, H, SEED = 256, 16, 3


# ------------------------------------------------------------------ scenes (built once, read-only)
def _costmap(size, seed=1):
    """uniform(0, 1) with a tenth of the cells at 0.995, above the default collision threshold."""
    rng = np.random.default_rng(seed)
    cm = rng.uniform(0.0, 1.0, (size, size)).astype(F32)
    cm[rng.uniform(size=cm.shape) < 0.1] = 0.995
    return cm


def _terrain(rows, cols, res, x_min, y_min):
    """Craters (scene.crater_dem's formula, the 9 craters at a quarter of their size) sampled on the
    cells of a rows x cols grid placed by x_min / y_min: not symmetric under a swap of x and y."""
    x = x_min + res * np.arange(cols)
    y = -y_min - res * np.arange(rows)
    X, Y = np.meshgrid(x, y)
    Z = np.zeros_like(X)
    for (cx, cy), h, w in scene.BUMPS_9:
        cx, cy, w = cx * 0.25, cy * 0.25, w * 0.25
        r2 = (X - cx) ** 2 + (Y - cy) ** 2
        Z += (h - 0.5) * np.exp(-r2 / (2 * w ** 2)) - (h + 0.5) * np.exp(-r2 / (2 * (w / 2) ** 2))
    return Z.astype(F32)


RESOLUTIONS = {                       # name -> (grid, scene_for's geometry)
    "0.1": (203, dict(half_width=10.15)),
    "0.07": (285, dict(half_width=9.975, resolution=0.07, x_min=-9.975, y_min=-9.975)),
    "third": (120, dict(half_width=20.0)),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "base":
        sc = hp.scene_for(scene.crater_dem(160, 20.0, scale=0.25), _costmap(37), 20.0)
    elif name == "nonsquare":         # x in [-30, 20], y in [-20, 10]
        sc = hp.scene_for(_terrain(120, 200, 0.25, -30.0, -10.0), _costmap(64), 30.0, resolution=0.25,
                          x_min=-30.0, y_min=-10.0)
    elif name == "transposed":        # x in [-30, 0], y in [-40, 10]
        sc = hp.scene_for(_terrain(200, 120, 0.25, -30.0, -10.0), _costmap(64), 30.0, resolution=0.25,
                          x_min=-30.0, y_min=-10.0)
    elif name.startswith("res/"):     # res/<resolution>/<costmap size>
        _, r, size = name.split("/")
        grid, geo = RESOLUTIONS[r]
        hw = geo["half_width"]
        cm = _costmap(int(size)) if int(size) > 1 else np.full((1, 1), 0.3, F32)
        sc = hp.scene_for(scene.crater_dem(grid, hw, scale=hw / 80.0), cm, **geo)
    elif name == "small_costmap":     # the costmap covers +-8 of the DEM's +-20
        sc = hp.scene_for(scene.crater_dem(160, 20.0, scale=0.25), _costmap(50), 20.0, cm_half_width=8.0)
    elif name == "min_dem":
        sc = hp.scene_for(np.array([[0.0, 0.3], [0.1, -0.2]], F32), np.full((1, 1), 0.3, F32), 20.0)
    else:
        raise KeyError(name)
    for a in (sc.Z, sc.costmap):
        a.setflags(write=False)
    return sc


# ------------------------------------------------------------------ a case
@dataclasses.dataclass(frozen=True)
class Case:
    scene: str = "base"
    params: tuple = ()                # R.Params / make_params overrides, as sorted (name, value) pairs
    state: tuple = ()                 # hp.oracle_state overrides
    K: int = K
    H: int = H
    proj: str = "3d"
    steps: int = 2

    def oracle_params(self):
        return R.Params(K=self.K, H=self.H, **{"seed": SEED, **dict(self.params)})

    def oracle_state(self):
        kw = {"x": START[0], "y": START[1], "goal": GOAL, **dict(self.state)}
        return hp.oracle_state(**kw)


def case(scene="base", state=None, K=K, H=H, proj="3d", steps=2, **params):
    return Case(scene, tuple(sorted(params.items())), tuple(sorted((state or {}).items())), K, H, proj, steps)


@functools.lru_cache(maxsize=None)
def _ref(c: Case):
    """The oracle's chain of c.steps steps, the nominal sequence fed back; every array finite."""
    p, sc, st = c.oracle_params(), _scene(c.scene), c.oracle_state()
    u1n, u2n = np.zeros(c.H, F32), np.zeros(c.H, F32)
    refs = []
    for step in range(c.steps):
        ref = R.mppi_step(p, sc, st, u1n, u2n, step, c.proj)
        part = ref["parts"][0]
        for name in ("cost",) + tuple(b for _, b in OUTS):
            assert np.isfinite(ref[name]).all(), f"{c}: the oracle's {name} of step {step} is not finite"
        for name in DUMPS:
            assert np.isfinite(part[name]).all(), f"{c}: the oracle's rollouts ({name}) of step {step} are not finite"
        refs.append(ref)
        u1n, u2n = ref["u1_opt"], ref["u2_opt"]
    return refs


def _parts(c: Case):
    """The oracle's K rollouts of every step of the case."""
    return [r["parts"][0] for r in _ref(c)]


def _oracle_terms(p, sc, st, part):
    """(terms [K, 4], collisions [K]): each critic from R.critics with its weight 1 and the others 0."""
    args = (sc, st, part["traj"], part["lw"], part["rw"], part["v"])
    terms = np.stack([R.critics(dataclasses.replace(p, **{w: (1.0 if w == one else 0.0) for w in WEIGHTS}), *args)
                      for one in WEIGHTS], -1)
    col = (R.costmap_at(sc, part["traj"][:, :, 0], part["traj"][:, :, 1]) > p.f("collision_threshold")).sum(1)
    assert np.isfinite(terms).all()
    return terms, col.astype(np.int32)


def _recombine(p, terms):
    cost = p.f("w_path") * terms[:, 0]
    cost = cost + p.f("w_slope") * terms[:, 1]
    cost = cost + p.f("w_speed") * terms[:, 2]
    cost = cost + p.f("w_obstacle") * terms[:, 3]
    return cost.astype(F32)


def _same(tag, name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{tag} {name}: shape {got.shape} vs {want.shape}"
    assert np.array_equal(got, want), hp.mismatch_report(f"{tag} {name}", got, want)


def _engine(c: Case, mode, monkeypatch, options=()):
    from mppi_amd import _lib
    if mode == "server":
        assert c.proj == "3d"
        monkeypatch.delenv("MPPI_ROLES", raising=False)
    else:
        monkeypatch.setenv("MPPI_ROLES", "1" if mode == "roles" else "0")
    eng = _lib.Engine(_lib.make_params(c.K, c.H, **{"seed": SEED, **dict(c.params)}), 0)
    try:
        for name, value in options:   # before the scene: the option must also hold for later set_dem / set_costmap
            eng.set_option(name, value)
        hp.bind_scene(eng, _scene(c.scene))
        eng.set_state(hp.state_for(c.oracle_state()))
        if mode == "server":
            eng.set_option("resident", 2)
            eng.set_option("resident_idle_us", 100000)
        else:
            eng.set_option("resident", 0)
    except BaseException:
        eng.close()
        raise
    return eng


def _run(c: Case, mode, monkeypatch, options=(), tag=None):
    """Run the case in one mode, compare everything with the oracle; returns what the engine gave."""
    refs = _ref(c)
    p, sc, st = c.oracle_params(), _scene(c.scene), c.oracle_state()
    tag = tag or f"{c.scene} {dict(c.params)} {dict(c.state)} K={c.K} H={c.H} {c.proj} {mode}"
    eng = _engine(c, mode, monkeypatch, options)
    got = {}
    try:
        for step, ref in enumerate(refs):
            eng.step(c.proj, step, copy=False)
            out = eng.outputs()
            for a, b in OUTS:
                _same(tag, f"step {step} {a}", out[a], ref[b])
                got[f"{step}/{a}"] = out[a]
        info = eng.launch_info()
        if mode == "server":   # a shape that fell back to separate launches must not pass
            assert info["resident"] == 1 and info["server_steps"] == c.steps, info
            assert info["server_failed_steps"] == 0 and info["server_fallbacks"] == 0, info
        else:
            assert info["resident"] == 0 and info["server_steps"] == 0, info
        # which division the cell indices took: the verified reciprocals (DEM 1 + costmap 2) unless switched off
        assert info["verified_reciprocals"] == (3 if dict(options).get("verified_reciprocal", 1) else 0), info
        got["cost"] = eng.costs()
        _same(tag, "cost", got["cost"], refs[-1]["cost"])
        d = eng.dump()
        part = refs[-1]["parts"][0]
        for name in DUMPS:
            _same(tag, f"dump {name}", d[name], part[name])
            got[f"dump/{name}"] = d[name]
        terms, col = eng.cost_terms()
        want_terms, want_col = _oracle_terms(p, sc, st, part)
        _same(tag, "terms", terms, want_terms)
        _same(tag, "collisions", col, want_col)
        _same(tag, "recombined terms", _recombine(p, terms), got["cost"])
        got["terms"], got["collisions"] = terms, col
    finally:
        eng.close()
    return got


def _modes(c: Case):
    return MODES if c.proj == "3d" else MODES_2D


# ------------------------------------------------------------------ parameter cases
ANGLE = dict(v_min_angular=-40.0, v_max_angular=40.0, dt=0.2, robot_radius=0.1, filter_a=0.5)
SIG08 = dict(s1=0.8, s2=0.8)
SIG05 = dict(s1=0.5, s2=0.5)
LARGE_ANGLE = case(state=SIG08, **ANGLE)
REVERSE = case(state=dict(heading=(-0.3, -0.9, 0.2), **SIG05), v_min_linear=-1.5)
LIMITS = case(state=SIG05, min_u1=-0.2, max_u1=0.6, min_u2=-0.9, max_u2=0.3)


def _small_angle_rule(c: Case):
    """fill_rollout's rule, in float32 like the host's: max(|wmin|, |wmax|) * dt < 0.78."""
    p = c.oracle_params()
    return bool(F32(max(abs(p.f("v_min_angular")), abs(p.f("v_max_angular")))) * p.f("dt") < F32(0.78))


def _w_all(c: Case):
    return np.concatenate([part["w"].ravel() for part in _parts(c)])


def _pre_large_angle(c: Case):
    assert not _small_angle_rule(c), "the case is on the small-angle arm"
    p, w = c.oracle_params(), _w_all(c)
    octant = (np.abs(w * p.f("dt")) * F32(4.0) / F32(np.pi)).astype(np.int64)
    counts = np.bincount(octant, minlength=11)
    assert octant.max() == 10 and (counts[:11] >= 100).all(), f"octants of |w dt|: {counts.tolist()}"
    assert (w > 0).any() and (w < 0).any()
    at_bound = np.abs(w) == F32(40.0)
    assert at_bound.mean() >= 0.01, f"{at_bound.mean():.3%} of |w| at the bound"


@pytest.mark.parametrize("mode", MODES)
def test_large_angle(mode, monkeypatch):
    """|w dt| up to 8 rad: the range-reduced dm_sincosf arm of both rollout kernels, every octant 0..10."""
    _pre_large_angle(LARGE_ANGLE)
    _run(LARGE_ANGLE, mode, monkeypatch)


EDGE = dict(robot_radius=0.2, filter_a=0.5)
EDGE_SMALL = case(state=SIG08, v_min_angular=-17.33, v_max_angular=17.33, **EDGE)   # 17.33 * 0.045 = 0.77985
EDGE_FULL = case(state=SIG08, v_min_angular=-17.34, v_max_angular=17.34, **EDGE)    # 17.34 * 0.045 = 0.7803
EDGE_PAST = case(state=SIG08, v_min_angular=-18.0, v_max_angular=18.0, **EDGE)      # 18 * 0.045 = 0.81 > pi / 4
EDGES = {"small": EDGE_SMALL, "full": EDGE_FULL, "past": EDGE_PAST}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("side", list(EDGES))
def test_angle_edge(side, mode, monkeypatch):
    """Just under and just over the 0.78 threshold, with rollouts clamped to the angular bound itself:
    the small-angle sin / cos at its largest argument, the general one at its smallest bound.  Up to
    pi / 4 the two give the same bits, so only the rule's own value tells the first two apart; "past"
    is the first bound (in steps of 0.2 rad/s) at which they differ: a threshold loosened that far fails."""
    from oracle import dmath
    c = EDGES[side]
    p = c.oracle_params()
    assert _small_angle_rule(c) == (side == "small")
    w, bound = _w_all(c), p.f("v_max_angular")
    at_bound = np.abs(w) == bound
    assert at_bound.mean() >= 0.01 and (w == bound).any() and (w == -bound).any(), f"{at_bound.mean():.3%} at the bound"
    angle = np.array([bound * p.f("dt")], F32)
    differ = not all(np.array_equal(a, b) for a, b in zip(dmath.dm_sincosf(angle), dmath.dm_sincosf_small(angle)))
    assert differ == (side == "past"), "the two sin / cos arms at the bound itself"
    _run(c, mode, monkeypatch)


def _pre_reverse(c: Case):
    v = np.concatenate([part["v"].ravel() for part in _parts(c)])
    assert (v < 0).mean() >= 0.25 and (v > 0).mean() >= 0.25, f"v < 0: {(v < 0).mean():.1%}, v > 0: {(v > 0).mean():.1%}"
    assert not (v + F32(0.0001) == 0).any(), "the speed critic divides by zero"


@pytest.mark.parametrize("mode", MODES)
def test_reverse(mode, monkeypatch):
    """v_min_linear < 0: v of either sign in the position update, the speed critic and the plan's reach."""
    _pre_reverse(REVERSE)
    _run(REVERSE, mode, monkeypatch)


def _pre_limits(c: Case):
    p = c.oracle_params()
    for part in _parts(c):
        for u, lo, hi in ((part["u1"], "min_u1", "max_u1"), (part["u2"], "min_u2", "max_u2")):
            for bound in (lo, hi):
                share = (u == p.f(bound)).mean()
                assert share >= 0.01, f"{share:.2%} of the samples on {bound}"
            assert (u >= p.f(lo)).all() and (u <= p.f(hi)).all()


@pytest.mark.parametrize("mode", MODES)
def test_control_limits(mode, monkeypatch):
    _pre_limits(LIMITS)
    _run(LIMITS, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES_2D)
@pytest.mark.parametrize("which", ["large_angle", "reverse", "limits"])
def test_2d(which, mode, monkeypatch):
    base, pre = {"large_angle": (LARGE_ANGLE, _pre_large_angle), "reverse": (REVERSE, _pre_reverse),
                 "limits": (LIMITS, _pre_limits)}[which]
    c = dataclasses.replace(base, proj="2d")
    pre(c)
    _run(c, mode, monkeypatch)


WHEELS = case(wheel_offset=0.45, robot_radius=0.8)
WHEELS_NEG = case(wheel_offset=-0.2)
WHEELS_POS = case()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["wide", "negative"])
def test_wheels(which, mode, monkeypatch):
    if which == "wide":
        c = WHEELS
        part = _parts(c)[-1]
        assert (part["lw"][..., :2] != part["rw"][..., :2]).any(axis=-1).all(), "a wheel pair coincides"
    else:   # the first step has the same rollouts whatever the offset: the wheels change sides
        c = WHEELS_NEG
        neg, pos = _parts(c)[0], _parts(WHEELS_POS)[0]
        assert np.array_equal(neg["traj"], pos["traj"]) and np.array_equal(neg["hv"], pos["hv"])
        assert np.array_equal(neg["lw"], pos["rw"]) and np.array_equal(neg["rw"], pos["lw"])
        assert not np.array_equal(neg["lw"], neg["rw"])
    _run(c, mode, monkeypatch)


def _dist_vs_horizon(c: Case):
    p, st = c.oracle_params(), c.oracle_state()
    xd, yd = F32(st.goal_x) - F32(st.x), F32(st.goal_y) - F32(st.y)
    return np.sqrt(xd * xd + yd * yd), p.horizon_f32()


NEAR_GOAL = dict(goal=(-6.0, -3.0))   # 6 m from the start
TIME_STEP = {
    "default_far": (case(dt=0.1, H=24), True),                                      # dt vmax H = 4.8 < 28 m
    "explicit_4_far": (case(dt=0.1, H=24, horizon=4.0, state=NEAR_GOAL), True),     # 6 > 4 (and 6 > 4.8)
    "explicit_8_near": (case(dt=0.1, H=24, horizon=8.0, state=NEAR_GOAL), False),   # 6 < 8 although 6 > 4.8
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(TIME_STEP))
def test_time_step_and_horizon(which, mode, monkeypatch):
    c, far = TIME_STEP[which]
    dist, horizon = _dist_vs_horizon(c)
    assert bool(dist > horizon) == far, (dist, horizon)
    if which != "default_far":
        assert dist > F32(0.1) * F32(2.0) * F32(24), "the default horizon would not tell the two cases apart"
        assert dist >= F32(2.0), "the speed critic is off"
    _run(c, mode, monkeypatch)


# The start (-12, -3) lies on a costmap cell of 0.80 that no default-speed rollout leaves (the cells are
# 1.08 m wide), so every rollout would collide: the case starts one cell to the right (0.46), 0.25 m from
# that cell's border, and drives left into it at 1 m/s.
COLLISION = case(collision_threshold=0.5, collision_penalty=777.0, w_slope=0.0, w_obstacle=3.0,
                 state=dict(x=-11.1, heading=(-1.0, 0.0, 0.0), wl=1.0, wr=1.0))


@pytest.mark.parametrize("mode", MODES)
def test_collision_rule(mode, monkeypatch):
    c = COLLISION
    p, sc = c.oracle_params(), _scene(c.scene)
    for part in _parts(c):
        col = (R.costmap_at(sc, part["traj"][..., 0], part["traj"][..., 1]) > p.f("collision_threshold")).sum(1)
        assert (col > 0).mean() >= 0.05 and (col == 0).mean() >= 0.05, f"colliding rollouts: {(col > 0).mean():.1%}"
    _run(c, mode, monkeypatch)


FILTER_0 = case(filter_a=0.0, opt_filter_a=0.0)
FILTER_1 = case(filter_a=1.0, opt_filter_a=1.0, state=dict(wl=0.7, wr=0.9))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("a", [0, 1])
def test_filter_edges(a, mode, monkeypatch):
    c = FILTER_1 if a else FILTER_0
    p = c.oracle_params()
    for ref in _ref(c):
        part = ref["parts"][0]
        if a:    # the wheels keep their speeds: v = 0.8, w = 0.2 / 1.2 at every step of every rollout
            v0, w0 = R.wheel_filter(p, c.oracle_state(), np.zeros((1, 1), F32), np.zeros((1, 1), F32), 3.5, 1.0)
            assert v0[0, 0] > 0 and w0[0, 0] > 0
            assert (part["v"] == v0[0, 0]).all() and (part["w"] == w0[0, 0]).all()
            assert (ref["v_opt"] == v0[0, 0]).all() and (ref["w_opt"] == w0[0, 0]).all()
        else:    # no memory: v follows the sample of the same step alone
            want = R.clampf(((part["u1"] * F32(3.5)) + (part["u2"] * F32(3.5))) / F32(2.0), F32(0.0), F32(2.0))
            assert np.array_equal(part["v"], want) and np.unique(part["v"]).size > 100
    _run(c, mode, monkeypatch)


SIGMA_0 = case(state=dict(s1=0.0, s2=0.0, wl=1.0, wr=1.3))


@pytest.mark.parametrize("mode", MODES)
def test_sigma_zero(mode, monkeypatch):
    """All K rollouts identical: every softmax weight is 1 and every 64-lane group of the leaf is live."""
    c = SIGMA_0
    refs = _ref(c)
    for ref in refs:
        assert np.unique(ref["cost"]).size == 1, "more than one distinct cost"
        part = ref["parts"][0]
        assert (part["traj"] == part["traj"][0]).all()
    assert np.array_equal(refs[0]["u1_opt"], np.zeros(c.H, F32)), "step 0's mean of identical zero samples"
    assert np.array_equal(refs[1]["parts"][0]["u1"][5], refs[0]["u1_opt"][np.minimum(np.arange(c.H) + 1, c.H - 1)])
    _run(c, mode, monkeypatch)


HEADINGS = [(-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.6, 0.0, 0.8), (-0.3, -0.9, 0.2)]


@pytest.mark.parametrize("mode", MODES_2D)
@pytest.mark.parametrize("moving", [False, True], ids=["at_rest", "moving"])
@pytest.mark.parametrize("heading", HEADINGS, ids=lambda h: "h" + "_".join(f"{v:g}" for v in h))
def test_headings(heading, moving, mode, monkeypatch):
    """The other three quadrants and a z component: from rest (the defaults), and at 0.9 m/s, which takes
    the rollouts over a few more cells."""
    state = dict(heading=heading, wl=0.8, wr=1.0) if moving else dict(heading=heading)
    _run(case(state=state, steps=1), mode, monkeypatch)


# ------------------------------------------------------------------ geometry cases
def _inside_dem(sc, x, y):
    """Strictly inside the DEM's extent (dem_cell's unclamped indices are then in range too)."""
    x0, y_top, res = float(sc.x_min), -float(sc.y_min), float(sc.res)
    return (x > x0) & (x < x0 + res * sc.grid) & (y < y_top) & (y > y_top - res * sc.rows)


def _inside_costmap(sc, x, y):
    return (np.abs(x) < float(sc.hw)) & (np.abs(y) < float(sc.hw))


# The start (-25, -15) heading +y is 5 m from the left and the bottom edge, and a horizon reaches
# dt * vmax * H = 1.44 m: no rollout can leave from there.  It stays as the interior case; the edges are
# crossed from the corner itself, 0.2 m from both, driving at it with sigma 0.8.
CORNER = dict(x=-29.8, y=-19.8, heading=(-1.0, -1.0, 0.0), wl=0.3, wr=0.3, s1=0.8, s2=0.8)
GEOMETRY = {
    "nonsquare": case("nonsquare", state=dict(x=-25.0, y=-15.0, heading=(0.0, 1.0, 0.0), wl=0.8, wr=1.0)),
    "nonsquare_corner": case("nonsquare", state=CORNER),
    "transposed": case("transposed", state=dict(x=-25.0, y=-15.0, heading=(0.0, 1.0, 0.0), wl=0.8, wr=1.0)),
    "transposed_corner": case("transposed", state=dict(CORNER, y=-39.8)),
}


def _pre_corner(c: Case):
    sc = _scene(c.scene)
    x_left, y_bottom = float(sc.x_min), -float(sc.y_min) - float(sc.res) * sc.rows
    for part in _parts(c):
        x, y = part["traj"][..., 0], part["traj"][..., 1]
        left, bottom = (x < x_left).any(1), (y < y_bottom).any(1)
        inside = _inside_dem(sc, x, y).all(1)
        assert left.sum() >= 5 and bottom.sum() >= 5 and inside.mean() > 0.5, \
            f"left {left.sum()}, bottom {bottom.sum()}, inside {inside.mean():.1%}"
        assert (left & ~bottom).any() and (bottom & ~left).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(GEOMETRY))
def test_non_square_dem(which, mode, monkeypatch):
    """120 x 200 and 200 x 120 cells with x_min = -30, y_min = -10: rows, grid, x_min and y_min all differ."""
    c = GEOMETRY[which]
    sc = _scene(c.scene)
    assert sc.rows != sc.grid and sc.x_min != sc.y_min
    if which.endswith("corner"):
        _pre_corner(c)
    else:
        tr = _parts(c)[-1]["traj"]
        assert _inside_dem(sc, tr[..., 0], tr[..., 1]).all()
    _run(c, mode, monkeypatch)


def _res_case(r, size):
    hw = RESOLUTIONS[r][1]["half_width"]    # the same place on each map (START on the 20 m one)
    return case(f"res/{r}/{size}", state=dict(x=START[0] * hw / 20.0, y=START[1] * hw / 20.0, wl=0.8, wr=1.0))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [37, 160, 1])
@pytest.mark.parametrize("r", list(RESOLUTIONS))
def test_resolutions(r, size, mode, monkeypatch):
    """DEM resolutions 0.1 (203^2), 0.07 (285^2) and 1/3 (120^2), each under a coarser costmap, one
    as fine as the base DEM and a single cell."""
    c = _res_case(r, size)
    sc = _scene(c.scene)
    want = {"0.1": F32(20.3 / 203), "0.07": F32(0.07), "third": F32(40.0 / 120)}[r]
    assert sc.res == want and sc.size == size and sc.rows == sc.grid == RESOLUTIONS[r][0]
    tr = _parts(c)[-1]["traj"]
    assert _inside_dem(sc, tr[..., 0], tr[..., 1]).all()
    assert np.unique(R.dem_cell(sc, tr[..., 0], tr[..., 1])[0]).size >= 2, "the rollouts stay in one column"
    _run(c, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("r", ["0.1", "0.07"])
def test_resolutions_from_beside_the_map(r, mode, monkeypatch):
    """The start (-12, -3) itself on the two 10 m maps: 2 m left of them, so every column clamps and the rows do not."""
    c = case(f"res/{r}/37", state=dict(wl=0.8, wr=1.0))
    sc = _scene(c.scene)
    tr = _parts(c)[-1]["traj"]
    i, j = R.dem_cell(sc, tr[..., 0], tr[..., 1])
    assert (i == -1).all() and (j > 0).all() and (j < sc.rows - 1).all() and np.unique(j).size >= 2
    _run(c, mode, monkeypatch)


SMALL_COSTMAP = case("small_costmap", state=dict(x=7.7, y=3.0, wl=1.2, wr=1.4))   # the goal (15, 5) is outside


@pytest.mark.parametrize("mode", MODES)
def test_costmap_smaller_than_dem(mode, monkeypatch):
    c = SMALL_COSTMAP
    sc, st = _scene(c.scene), c.oracle_state()
    assert sc.hw == F32(8.0) and sc.x_min == F32(-20.0)
    assert _inside_costmap(sc, st.x, st.y) and not _inside_costmap(sc, st.goal_x, st.goal_y)
    for part in _parts(c):
        x, y = part["traj"][..., 0], part["traj"][..., 1]
        assert _inside_dem(sc, x, y).all()
        out = ~_inside_costmap(sc, x, y)
        crossed = out.any(1) & ~out.all(1)
        assert crossed.mean() > 0.25, f"{crossed.mean():.1%} of the rollouts cross the costmap's border"
    _run(c, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_minimum_dem_and_costmap(mode, monkeypatch):
    """2 x 2 DEM (a 3 x 3 normal table, every lookup clamped) under a 1 x 1 costmap."""
    c = case("min_dem", state=dict(wl=0.8, wr=1.0))
    sc = _scene(c.scene)
    assert (sc.rows, sc.grid, sc.size) == (2, 2, 1)
    _run(c, mode, monkeypatch)


OUTSIDE = case(state=dict(x=45.0, y=-33.0, wl=0.8, wr=1.0))


@pytest.mark.parametrize("mode", MODES)
def test_whole_horizon_outside_the_map(mode, monkeypatch):
    c = OUTSIDE
    sc = _scene(c.scene)
    for ref in _ref(c):
        part = ref["parts"][0]
        for tr in (part["traj"], part["lw"], part["rw"], ref["traj_sim"][None]):
            x, y = tr[..., 0], tr[..., 1]
            assert (x > 20.0).all() and (y < -20.0).all()
            assert not _inside_dem(sc, x, y).any() and not _inside_costmap(sc, x, y).any()
    _run(c, mode, monkeypatch)


IEEE = {"nonsquare": GEOMETRY["nonsquare_corner"], "res0.07": _res_case("0.07", 37)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", list(IEEE))
def test_ieee_cell_division(which, mode, monkeypatch):
    """mppi_set_option "verified_reciprocal" 0: the chains' copy without the reciprocal (CD = false,
    cdiv == 0 in Dem::cell / Dem::point / costmap_index) gives the oracle's bits and the bits of the
    same engine with the option at 1; set after the scene or before it, and switched back."""
    c = IEEE[which]
    if which == "nonsquare":
        _pre_corner(c)
    off = _run(c, mode, monkeypatch, options=(("verified_reciprocal", 0),), tag=f"{which} {mode} ieee")
    on = _run(c, mode, monkeypatch, options=(("verified_reciprocal", 0), ("verified_reciprocal", 1)),
              tag=f"{which} {mode} verified")
    assert off.keys() == on.keys()
    for name in off:
        _same(f"{which} {mode} ieee vs verified", name, off[name], on[name])
    # switched on a bound scene: off, a step, on again, a step
    eng = _engine(c, mode, monkeypatch)
    try:
        for value in (0, 1):
            eng.set_option("verified_reciprocal", value)
            eng.set_nominal(np.zeros(c.H, F32), np.zeros(c.H, F32))
            eng.step(c.proj, 0, copy=False)
            out = eng.outputs()
            assert eng.launch_info()["verified_reciprocals"] == 3 * value
            for a, b in OUTS:
                _same(f"{which} {mode} option {value} on a bound scene", a, out[a], _ref(c)[0][b])
            _same(f"{which} {mode} option {value} on a bound scene", "cost", eng.costs(), _ref(c)[0]["cost"])
    finally:
        eng.close()
