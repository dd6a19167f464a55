"""GPU: terrain, poses and costs that are not finite, against the oracle.

Every comparison is exact, with NaN == NaN (x86 makes the negative quiet NaN where the GPU makes the
positive one): `nonfinite_refs.assert_same`.  What D13 leaves open is not compared: the kind of a
dead cost (only that it is not finite), a dumped rollout array past its trajectory's first element
that is not finite, and the *_sim rows of a step whose pose holds +-inf (the cell an infinite
coordinate reads is unspecified).

  * chosen dead sets: step_injected with finite controls on a DEM whose far part is NaN / +inf /
    +-3e38; the controls drive exactly the intended trajectories into it (asserted on the oracle);
  * crafted records into mppi_step_finish: a whole member dead beside live ones;
  * sampled steps on the same DEMs and on a costmap with NaN / +inf / -inf cells, two chained steps,
    server and separate launches; the leaf record of mppi_step_partial;
  * a whole step without a usable pose, then recovery with the next good pose;
  * the drop-in MPPI_Controller with a NaN pose;
  * the standalone lookups and the path scorer.
"""
import functools
import warnings

import numpy as np
import pytest

import helpers as hp
import nonfinite_refs as N
from oracle import mppi_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

F32 = np.float32
T_SPARSE, T_DENSE = 0.3, 3000.0
OUT = dict(u1_opt="u1_opt", u2_opt="u2_opt", lin_vel="v_opt", ang_vel="w_opt", traj_sim="traj_sim",
           heading_sim="hv_sim", left_wheel_sim="lw_sim", right_wheel_sim="rw_sim")
CONTROLS = ("u1_opt", "u2_opt", "lin_vel", "ang_vel")
DUMPS = ("traj", "hv", "lw", "rw", "v", "w", "u1", "u2")
ORIGIN = dict(x=0.0, y=0.0, goal=(15.0, 2.0))


@pytest.fixture(params=["roles", "pair"])
def rollout_kernel(request, monkeypatch):
    """Both rollout kernels, forced by MPPI_ROLES, which a context reads when it is created."""
    monkeypatch.setenv("MPPI_ROLES", "1" if request.param == "roles" else "0")
    return request.param


def _zeros(H):
    return np.zeros(H, F32), np.zeros(H, F32)


def _freeze(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _oracle_step(p, sc, st, nominal, step, injected=None):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return _freeze(R.mppi_step(p, sc, st, nominal[0], nominal[1], step, injected=injected))


def _assert_costs(tag, got, want):
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), \
        f"{tag}: finiteness of {int((np.isfinite(got) != np.isfinite(want)).sum())} costs differs"
    fin = np.isfinite(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32)), \
        hp.mismatch_report(f"{tag} finite costs", got[fin], want[fin])


def _assert_outputs(tag, out, ref, names=tuple(OUT)):
    for a in names:
        N.assert_same(f"{tag} {a}", out[a], ref[OUT[a]])
    for a in CONTROLS:    # D13: what the step emits and hands on is finite whatever went in
        assert np.isfinite(out[a]).all() or not np.isfinite(ref[OUT[a]]).all(), f"{tag} {a} not finite"


def _assert_dump(tag, d, part):
    for name in DUMPS:
        spec = N.specified_prefix(part[name]) if part[name].ndim == 3 else np.isfinite(part[name])
        ok = N.same_bits_or_nan(d[name], part[name]) | ~spec
        assert ok.all(), N.nan_report(f"{tag} dump {name}", np.where(spec, d[name], 0), np.where(spec, part[name], 0))


# ================================================================== chosen dead sets
@functools.lru_cache(maxsize=None)
def _scene(kind, H, y_from=None):
    Z = N.patched_dem(kind, N.X_FROM[H], y_from)
    Z.setflags(write=False)
    return hp.scene_for(Z, N.flat_costmap(), N.HW)


@functools.lru_cache(maxsize=None)
def _chosen(K, H, pattern, kind, T):
    sc = _scene(kind, H)
    dead = N.dead_set(pattern, K)
    u1, u2 = N.chosen_controls(dead, H)
    st = hp.oracle_state(**ORIGIN)
    p = R.Params(K=K, H=H, temperature=T)
    ref = _oracle_step(p, sc, st, _zeros(H), 0, injected=(u1, u2))
    # the scene does what the case says, on the oracle alone
    assert np.array_equal(~np.isfinite(ref["cost"]), dead), f"dead set of {pattern} K={K} H={H} {kind} is not the intended one"
    assert np.isfinite(sc.Z[:, :int((N.X_FROM[H] + N.HW) * 10) - 1]).all()
    return sc, st, u1, u2, ref


def _run_chosen(K, H, pattern, kind, T, dump=False):
    sc, st, u1, u2, ref = _chosen(K, H, pattern, kind, T)
    tag = f"{pattern} {kind} K={K} H={H} T={T}"
    eng, _ = hp.engine_on(K, H, sc.Z, sc.costmap, st, N.HW, temperature=T)
    try:
        out = eng.step_injected(u1, u2)
        if H == 100:
            assert 0 < eng.launch_info()["ucache_steps"] < H   # rows past the control cache are re-read
        _assert_costs(tag, eng.costs(), ref["cost"])
        _assert_outputs(tag, out, ref)
        if N.dead_set(pattern, K).all():
            for a in ("u1_opt", "u2_opt"):
                assert np.array_equal(out[a].view(np.uint32), np.zeros(H, np.uint32)), f"{tag}: {a} is not +0.0"
        g1, g2 = eng.get_nominal()
        assert np.array_equal(g1.view(np.uint32), ref["u1_opt"].view(np.uint32))
        assert np.array_equal(g2.view(np.uint32), ref["u2_opt"].view(np.uint32))
        if dump:
            _assert_dump(tag, eng.dump(), ref["parts"][0])
    finally:
        eng.close()


@pytest.mark.parametrize("T", [T_SPARSE, T_DENSE], ids=["sparse", "dense"])
@pytest.mark.parametrize("pattern", N.PATTERNS)
@pytest.mark.parametrize("K", [256, 300, 1280])
def test_chosen_dead_sets(rollout_kernel, K, pattern, T):
    """Every dead set at every K and both leaf layouts; the patch kind goes round with the case, and
    test_patch_kinds crosses the kinds with the shapes once more."""
    kind = N.PATCH_KINDS[(N.PATTERNS.index(pattern) + [256, 300, 1280].index(K)) % 3]
    _run_chosen(K, 24, pattern, kind, T)


@pytest.mark.parametrize("kind", N.PATCH_KINDS)
@pytest.mark.parametrize("K", [256, 300, 1280])
def test_patch_kinds(rollout_kernel, K, kind):
    """Each patch kind at each K (a dead half, sparse and dense), with the rollouts dumped at K = 300."""
    _run_chosen(K, 24, "half", kind, T_SPARSE, dump=(K == 300))
    _run_chosen(K, 24, "lane", kind, T_DENSE)


@pytest.mark.parametrize("pattern", ["line", "all-but-one", "all"])
def test_chosen_dead_sets_long_horizon(rollout_kernel, pattern):
    """K = 1280, H = 100: the leaf re-reads the rows past the control cache."""
    _run_chosen(1280, 100, pattern, N.PATCH_KINDS[N.PATTERNS.index(pattern) % 3], T_SPARSE)
    _run_chosen(1280, 100, pattern, "nan", T_DENSE)


# ================================================================== crafted records into the finish
def _crafted_records(n, H, kind, pos, seed):
    rng = np.random.RandomState(seed)
    recs = rng.uniform(-1.0, 1.0, (n, 2 * H + 2))
    recs[:, 0] = 40.0 + rng.uniform(0.0, 1.0, n).astype(F32)      # m: a float32 value
    recs[:, 1] = rng.uniform(0.5, 200.0, n)
    if kind == "all-empty":
        recs[:] = R.empty_record(H)
    elif kind == "S=0":
        recs[pos] = 0.0
        recs[pos, 0] = 39.5
    else:   # not finite: S and V are not read beside a live member; alone they are 0 (D13)
        if n == 1:
            recs[pos] = 0.0
        recs[pos, 0] = dict(nan=float(N.POS_NAN), neg_nan=float(N.NEG_NAN), inf=np.inf)[kind]
    return recs


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_finish_with_dead_members(n):
    """mppi_step_finish on n records of which one is dead: m NaN (both signs), +inf, or finite with
    S = 0, at the first, the middle and the last place, and all empty; against tree_reduce + finish."""
    import torch
    K, H, T = 256, 12, T_SPARSE
    sc = _scene("nan", 24)
    st = hp.oracle_state(**ORIGIN)
    p = R.Params(K=K, H=H, temperature=T)
    eng, _ = hp.engine_on(K, H, sc.Z, sc.costmap, st, N.HW, temperature=T)
    try:
        assert eng.record_len() == 2 * H + 2
        cases = [(kind, pos) for kind in ("nan", "neg_nan", "inf", "S=0") for pos in sorted({0, n // 2, n - 1})]
        for i, (kind, pos) in enumerate(cases + [("all-empty", 0)]):
            recs = _crafted_records(n, H, kind, pos, seed=i)
            with np.errstate(all="ignore"):
                root = R.tree_reduce(recs, T)
                ref = R.finish(p, sc, st, root)
            dev = torch.from_numpy(recs).cuda()
            out = eng.step_finish(dev.data_ptr(), n)
            tag = f"n={n} {kind}@{pos}"
            _assert_outputs(tag, out, ref)
            if kind == "all-empty" or n == 1:    # nothing live: +0.0 everywhere
                for a in ("u1_opt", "u2_opt"):
                    assert np.array_equal(out[a].view(np.uint32), np.zeros(H, np.uint32)), f"{tag}: {a} is not +0.0"
            else:
                assert ref["u1_opt"].any() and ref["u2_opt"].any(), tag
    finally:
        eng.close()


# ================================================================== sampled steps
def _assert_mixed(cost, tag):
    """The share of dead costs lies in [0.2, 0.8] and some leaf holds both kinds (on the oracle)."""
    dead = ~np.isfinite(cost)
    assert 0.2 <= dead.mean() <= 0.8, f"{tag}: dead share {dead.mean():.3f}"
    pad = np.concatenate([dead, np.ones(-dead.size % R.LEAF, bool)]).reshape(-1, R.LEAF)
    live = np.concatenate([~dead, np.zeros(-dead.size % R.LEAF, bool)]).reshape(-1, R.LEAF)
    assert (pad.any(axis=1) & live.any(axis=1)).any(), f"{tag}: no leaf holds both dead and live costs"


def _sampled_scene(what):
    """(scene, state).  The rover rolls at 1 m/s and the sampled fan ends 0.5 .. 0.85 m ahead: the DEM
    patch begins where the faster part of it arrives; or a 0.1 m costmap whose cells from there on
    are +inf (right of the axis), -inf (the 0.1 m strip left of it) and NaN (further left): costs of
    all three kinds, -inf among them (D13: reachable, and dead)."""
    if what in N.PATCH_KINDS:
        Z = N.patched_dem(what, 0.72)
        cm = N.flat_costmap()
    else:
        Z = N.base_dem()
        cm = np.random.RandomState(4).uniform(0.0, 0.9, (N.GRID, N.GRID)).astype(F32)
        xs = (np.arange(N.GRID) + 0.5) * (2.0 * N.HW / N.GRID) - N.HW
        X, Y = np.meshgrid(xs, -xs)
        cm[(X > 0.7) & (Y > 0.0)] = F32(-np.inf)    # the strip 0 <= y < 0.1
        cm[(X > 0.7) & (Y > 0.1)] = N.POS_NAN
        cm[(X > 0.7) & (Y <= 0.0)] = F32(np.inf)
    return hp.scene_for(Z, cm, N.HW), hp.oracle_state(s1=0.5, s2=0.5, wl=1.0, wr=1.0, **ORIGIN)


@functools.lru_cache(maxsize=None)
def _sampled(what, K, H, T, seed, steps=2):
    sc, st = _sampled_scene(what)
    p = R.Params(K=K, H=H, temperature=T, seed=seed)
    nominal, refs = _zeros(H), []
    for i in range(steps):
        ref = _oracle_step(p, sc, st, nominal, i)
        _assert_mixed(ref["cost"], f"{what} seed {seed} step {i}")
        if what == "costmap":
            c = ref["cost"]
            assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any(), "costmap: a kind is missing"
        nominal = (ref["u1_opt"], ref["u2_opt"])
        refs.append(ref)
    return sc, st, refs


@pytest.mark.parametrize("resident", [2, 0], ids=["server", "separate"])
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("what", N.PATCH_KINDS + ("costmap",))
def test_sampled_steps(monkeypatch, what, seed, resident):
    """Two chained sampled steps at K = 1280, H = 24 with 20 .. 80 % of the costs dead and a leaf that
    holds both kinds (asserted on the oracle), on the resident server and as separate launches."""
    monkeypatch.setenv("MPPI_ROLES", "1")
    K, H, T = 1280, 24, T_SPARSE if seed == 0 else T_DENSE
    sc, st, refs = _sampled(what, K, H, T, seed)
    eng, _ = hp.engine_on(K, H, sc.Z, sc.costmap, st, N.HW, temperature=T, seed=seed)
    eng.set_option("resident", resident)
    try:
        for i, ref in enumerate(refs):
            out = eng.step("3d", i)
            tag = f"{what} seed {seed} step {i}"
            _assert_costs(tag, eng.costs(), ref["cost"])
            _assert_outputs(tag, out, ref)
            g1, g2 = eng.get_nominal()
            assert np.isfinite(g1).all() and np.isfinite(g2).all()
        info = eng.launch_info()
        assert info["resident"] == (1 if resident else 0), info
        if resident:
            assert info["server_steps"] == len(refs) and info["server_failed_steps"] == 0, info
        _assert_dump(tag, eng.dump(), refs[-1]["parts"][0])
    finally:
        eng.close()


@pytest.mark.parametrize("K", [256, 1280])
@pytest.mark.parametrize("what", N.PATCH_KINDS + ("costmap",))
def test_step_partial_record(rollout_kernel, what, K):
    """The record of mppi_step_partial: m, S and every V with NaN == NaN (D13 leaves no NaN in it)."""
    import torch
    H, T = 24, T_SPARSE
    sc, st = _sampled_scene(what)
    p = R.Params(K=K, H=H, temperature=T, seed=3)
    with np.errstate(all="ignore"):
        want, r = R.shard_record(p, sc, st, *_zeros(H), 0, 0, K)
    _assert_mixed(r["cost"], f"{what} K={K}")
    assert np.isfinite(want).all()
    eng, _ = hp.engine_on(K, H, sc.Z, sc.costmap, st, N.HW, temperature=T, seed=3)
    try:
        rec = torch.empty(eng.record_len(), dtype=torch.float64, device="cuda:0")
        eng.step_partial(rec.data_ptr(), "3d", 0)
        torch.cuda.synchronize()
        N.assert_same(f"record {what} K={K}", rec.cpu().numpy(), want)
    finally:
        eng.close()


def test_dead_leaf_record_is_the_empty_record(rollout_kernel):
    """A leaf without a finite cost writes m = +inf, S = 0, V = 0, not a NaN minimum (K = 256: no padding
    lane supplies the +inf)."""
    import torch
    K, H = 256, 9
    sc = hp.scene_for(N.base_dem(), N.flat_costmap(), N.HW)
    st = hp.oracle_state(x=float("nan"), y=0.0, goal=ORIGIN["goal"])
    with np.errstate(all="ignore"):
        want, r = R.shard_record(R.Params(K=K, H=H), sc, st, *_zeros(H), 0, 0, K)
    assert not np.isfinite(r["cost"]).any()
    assert np.array_equal(want.view(np.int64), R.empty_record(H).view(np.int64))
    eng, _ = hp.engine_on(K, H, sc.Z, sc.costmap, st, N.HW)
    try:
        rec = torch.empty(eng.record_len(), dtype=torch.float64, device="cuda:0")
        eng.step_partial(rec.data_ptr(), "3d", 0)
        torch.cuda.synchronize()
        got = rec.cpu().numpy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), hp.mismatch_report("record", got, want)
    finally:
        eng.close()


# ================================================================== a whole step without a usable pose
GOOD = dict(wl=0.2, wr=0.25, **ORIGIN)
# name -> (the state's fields, dead: no finite cost on the oracle, sim: the *_sim rows are specified)
BAD_STATES = {
    "nan-x": (dict(GOOD, x=float("nan")), True, True),
    "inf-y": (dict(GOOD, y=float("inf")), True, False),          # an infinite coordinate reads an unspecified cell
    "zero-heading": (dict(GOOD, heading=(0.0, 0.0, 0.0)), True, True),
    # D13: clamp(NaN) is the lower bound, so the filter turns NaN wheel speeds into (v_min, w_min) and
    # the trajectories live; and a goal whose distance overflows takes the far branch with finite terms
    "nan-wheels": (dict(GOOD, wl=float("nan"), wr=float("nan")), False, True),
    "goal-1e30": (dict(GOOD, goal=(1e30, 0.0)), False, True),
}


@pytest.mark.parametrize("resident", [2, 0], ids=["server", "separate"])
@pytest.mark.parametrize("bad", list(BAD_STATES))
def test_bad_state_then_recovery(monkeypatch, bad, resident):
    """One step with a state that is not finite (K = 300, H = 9), then set_state with the good one and
    two more steps: every output equals the oracle's continuation from the nominal sequence the bad step
    handed over.  Where the oracle has no finite cost, u_opt is +0.0.  Nothing stays NaN."""
    monkeypatch.setenv("MPPI_ROLES", "1")
    K, H = 300, 9
    fields, dead, sim = BAD_STATES[bad]
    sc = hp.scene_for(N.base_dem(), N.flat_costmap(), N.HW)
    with np.errstate(all="ignore"):
        st_bad, st_good = hp.oracle_state(**fields), hp.oracle_state(**GOOD)
    p = R.Params(K=K, H=H, seed=5)
    ref0 = _oracle_step(p, sc, st_bad, _zeros(H), 0)
    assert (not np.isfinite(ref0["cost"]).any()) == dead, f"{bad}: the oracle's step is {'not ' if dead else ''}dead"
    with np.errstate(all="ignore"):
        eng, _ = hp.engine_on(K, H, sc.Z, sc.costmap, st_bad, N.HW, seed=5)
    eng.set_option("resident", resident)
    try:
        out = eng.step("3d", 0)
        _assert_costs(bad, eng.costs(), ref0["cost"])
        _assert_outputs(bad, out, ref0, tuple(OUT) if sim else CONTROLS)
        if dead:
            for a in ("u1_opt", "u2_opt"):
                assert np.array_equal(out[a].view(np.uint32), np.zeros(H, np.uint32)), f"{bad}: {a} is not +0.0"
        if bad != "nan-wheels":   # (the filter's own state is the NaN wheel speed there; the command is clamped)
            assert np.isfinite(out["lin_vel"]).all() and np.isfinite(out["ang_vel"]).all()
        nominal = (ref0["u1_opt"], ref0["u2_opt"])
        assert np.isfinite(nominal[0]).all() and np.isfinite(nominal[1]).all()
        eng.set_state(hp.state_for(st_good))
        for i in (1, 2):
            ref = _oracle_step(p, sc, st_good, nominal, i)
            assert np.isfinite(ref["cost"]).all()
            out = eng.step("3d", i)
            tag = f"{bad} recovery step {i}"
            assert np.array_equal(eng.costs().view(np.uint32), ref["cost"].view(np.uint32)), tag
            for a in OUT:
                assert np.array_equal(out[a].view(np.uint32), ref[OUT[a]].view(np.uint32)), \
                    hp.mismatch_report(f"{tag} {a}", out[a], ref[OUT[a]])
            nominal = (ref["u1_opt"], ref["u2_opt"])
        info = eng.launch_info()
        assert info["resident"] == (1 if resident else 0) and info["server_failed_steps"] == 0, info
    finally:
        eng.close()


def test_controller_with_a_nan_pose():
    """The drop-in MPPI_Controller: a NaN pose gives the command (0, 0) of an all-dead step, and the
    next good pose the oracle's step from a zero nominal sequence."""
    import yaml
    from mppi_amd.controller import DEFAULT_CONFIG, MPPI_Controller, Robot, Surface
    K, H = 300, 12
    with open(DEFAULT_CONFIG) as f:
        cfg = yaml.safe_load(f)
    cfg["controller"]["number_of_trajectories"] = K
    cfg["controller"]["number_of_iterations"] = H
    Z, cm = N.base_dem(), N.flat_costmap()
    robot = Robot(0.0, 0.0, [1.0, 0.0, 0.0], cfg)
    ctl = MPPI_Controller(Surface.from_arrays(Z, cm, N.HW), robot, cfg, 15.0, 2.0, 0.0)
    ctl.warp_setup()
    robot.update_position(float("nan"), 0.0, 0.0, robot.heading_vector)
    v0, w0 = ctl.step("3d")
    assert (v0, w0) == (0.0, 0.0)
    assert not ctl.optimal_u1_wp.numpy().any() and not np.isfinite(ctl.costs_wp.numpy()).any()
    robot.update_position(0.0, 0.0, 0.0, robot.heading_vector)
    v1, w1 = ctl.step("3d")
    st = R.State(x=0.0, y=0.0, goal_x=15.0, goal_y=2.0, std_dev_u1=float(ctl.std_dev_u1), std_dev_u2=float(ctl.std_dev_u2))
    ref = R.mppi_step(R.Params(K=K, H=H, seed=42), R.Scene(Z, N.HW, cm), st, *_zeros(H), 1)
    np.testing.assert_array_equal(ctl.costs_wp.numpy(), ref["cost"])
    np.testing.assert_array_equal(ctl.optimal_u1_wp.numpy(), ref["u1_opt"])
    assert (v1, w1) == (float(ref["v_opt"][0]), float(ref["w_opt"][0])) and np.isfinite([v1, w1]).all()


# ================================================================== standalone lookups and the scorer
SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38], F32)


@pytest.mark.parametrize("which", ["odd", "non_square"])
def test_lookups_with_nonfinite_queries(which):
    """bilinear_query, bin_queries and bilinear_tiled with NaN, +-inf and +-3e38 among the queries (first,
    last and scattered, on either axis and on both): off and perm stay a partition and a permutation,
    heights equal R.bilinear with NaN == NaN, tiled equals scattered."""
    import torch
    from mppi_amd import _lib
    n = 20_003
    if which == "odd":
        Z, hw, geo = np.random.default_rng(3).normal(size=(203, 203)).astype(F32), 10.15, {}
        lo, hi = (-15.0, -15.0), (15.0, 15.0)
    else:
        Z, hw, geo = np.random.default_rng(5).normal(size=(120, 200)).astype(F32), 30.0, \
            dict(resolution=0.25, x_min=-30.0, y_min=-10.0)
        lo, hi = (-45.0, -35.0), (35.0, 25.0)
    rng = np.random.default_rng(21)
    x = rng.uniform(lo[0], hi[0], n).astype(F32)
    y = rng.uniform(lo[1], hi[1], n).astype(F32)
    where = np.concatenate([[0, 1, 2, n - 3, n - 2, n - 1], rng.choice(np.arange(3, n - 3), 600, replace=False)])
    for k, i in enumerate(where):
        s = SPECIALS[k % 6]
        if k % 3 != 1:
            x[i] = s
        if k % 3 != 0:
            y[i] = SPECIALS[(k // 6) % 6] if k % 3 == 2 else s
    sc = hp.scene_for(Z, np.zeros((4, 4), F32), hw, **geo)
    with np.errstate(all="ignore"):
        want = R.bilinear(x, y, R.get_corners_heights(sc, x, y), sc.res).astype(F32)
    assert np.isnan(want[where]).all() and np.isfinite(np.delete(want, where)).all()
    eng = _lib.Engine(_lib.make_params(256, 8), 0)
    try:
        eng.set_dem(Z, hw, **geo)
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        hd = torch.empty_like(xd)
        eng.bilinear_query(xd.data_ptr(), yd.data_ptr(), hd.data_ptr(), n)
        got = hd.cpu().numpy()
        N.assert_same("bilinear_query", got, want)
        nt = eng.bilinear_tiles()
        xs, ys = torch.empty_like(xd), torch.empty_like(xd)
        perm = torch.empty(n, dtype=torch.int32, device="cuda")
        off = torch.empty(nt + 1, dtype=torch.int32, device="cuda")
        eng.bin_queries(xd.data_ptr(), yd.data_ptr(), n, xs.data_ptr(), ys.data_ptr(), perm.data_ptr(), off.data_ptr())
        o, pm = off.cpu().numpy(), perm.cpu().numpy()
        assert o[0] == 0 and o[-1] == n and np.all(np.diff(o) >= 0)
        assert np.array_equal(np.sort(pm), np.arange(n))
        assert N.same_bits_or_nan(xs.cpu().numpy(), x[pm]).all() and N.same_bits_or_nan(ys.cpu().numpy(), y[pm]).all()
        ht = torch.empty_like(xd)
        eng.bilinear_tiled(xs.data_ptr(), ys.data_ptr(), off.data_ptr(), ht.data_ptr())
        eng.sync()
        tiled = np.empty(n, F32)
        tiled[pm] = ht.cpu().numpy()
        N.assert_same("tiled", tiled, got)
    finally:
        eng.close()


def test_score_paths_through_a_nan_patch():
    """Paths that enter a NaN patch of the DEM (heights and wheel contacts NaN from there on) over a
    costmap with NaN and +inf cells: cost, each term and the collision count per the oracle."""
    n, L = 65, 24
    sc = hp.scene_for(N.patched_dem("nan", N.X_FROM[L]), _sampled_scene("costmap")[0].costmap, N.HW)
    st = hp.oracle_state(**ORIGIN)
    p = R.Params(K=n, H=L)
    dead = np.arange(n) % 3 == 0
    u1, u2 = N.chosen_controls(dead, L, seed=2)
    with np.errstate(all="ignore"):
        v, w = R.wheel_filter(p, st, u1, u2, p.filter_k, p.filter_a)
        traj, _, lw, rw = R.rollout3d(p, sc, st, v, w)
        assert np.array_equal(np.isnan(traj[:, :, 2]).any(axis=1), dead)
        cost = R.critics(p, sc, st, traj, lw, rw, v)
        terms = np.stack(R.critic_terms(p, sc, st, traj, lw, rw, v), -1)
        col = (R.costmap_at(sc, traj[:, :, 0], traj[:, :, 1]) > p.f("collision_threshold")).sum(1).astype(np.int32)
    assert not np.isfinite(cost[dead]).any()
    eng, _ = hp.engine_on(256, L, sc.Z, sc.costmap, st, N.HW)
    try:
        got = eng.score_paths(traj, v, lw, rw, state=hp.state_for(st))
        N.assert_same("score cost", got["cost"], cost)
        N.assert_same("score terms", got["terms"], terms)
        assert np.array_equal(got["collisions"], col)
    finally:
        eng.close()
