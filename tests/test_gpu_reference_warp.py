"""GPU: the HIP engine against whole steps of the REFERENCE'S OWN Warp code.

tests/golden/ref_warp_steps.npz (tests/golden/make_warp_golden.py) holds what the
reference's kernels and host class computed under the project's Warp stand-in.  The tests read that
file alone.  One engine per case at the fixture's K and H, on both rollout kernels (MPPI_ROLES, as
tests/test_gpu_parity.py); every comparison with the reference-run arrays is bitwise, except the
emitted controls, which the engine sums in float64 in a fixed tree (D2) where the reference sums in
float32 in launch order: those are held to the project's 1e-5 (helpers.rel_err).

The tail.  The reference's optimal rollout is its rollout kernel on optimal_u* through the optimal
filter (k = 3.0, a = 0.92).  The engine's own *_sim arrays start from its float64 u_opt, which may
differ from the reference's float32 sum in the last bit, so they cannot be held bitwise to the
fixture.  Instead the engine rolls out the fixture's optimal_u* itself, with filter_k / filter_a set
to 3.0 / 0.92: injected as the controls of every trajectory, every rollout is the reference's optimal
rollout, bitwise.  (Sampled from set_nominal(optimal_u*) with sigma 0 the engine's rollouts are those
of the sequence SHIFTED by one, sampling_warp.py:71-92: that form pins the shift on the device.)
"""
import numpy as np
import pytest

import alt_critics_refs as A
import helpers as hp
import warp_golden as G

pytestmark = pytest.mark.gpu

F32 = np.float32
DUMPS = ("u1", "u2", "v", "w", "traj", "hv", "lw", "rw")
WEIGHTS = ("w_path", "w_slope", "w_speed", "w_obstacle")
W_ORIENTATION = 1000.0


@pytest.fixture(autouse=True, params=["roles", "pair"])
def rollout_kernel(request, monkeypatch):
    """Both rollout kernels, forced by MPPI_ROLES, which a context reads when it is created."""
    monkeypatch.setenv("MPPI_ROLES", "1" if request.param == "roles" else "0")
    return request.param


def _engine(c, state=None, **params):
    from mppi_amd import _lib
    sc = G.scene()
    eng = _lib.Engine(_lib.make_params(c.K, c.H, **G.params_kw(c, **params)), 0)
    try:
        eng.set_option("resident", 0)                # the two rollout kernels as separate launches
        hp.bind_scene(eng, sc)
        eng.set_state(G.engine_state(c) if state is None else state)
    except BaseException:
        eng.close()
        raise
    return eng


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{tag}: {got.dtype} {got.shape} vs {want.shape}"
    assert np.array_equal(got, want), hp.mismatch_report(tag, got, want)


def _recombine(c, terms):
    cost = c.p.f("w_path") * terms[:, 0]
    for i in (1, 2, 3):
        cost = cost + c.p.f(WEIGHTS[i]) * terms[:, i]
    return cost.astype(F32)


def _assert_step(c, eng, out):
    tag = c.name
    costs = eng.costs()
    _same(f"{tag} costs", costs, c.costs)
    d = eng.dump()
    for name in DUMPS:
        _same(f"{tag} dump {name}", d[name], getattr(c, name))
    terms, col = eng.cost_terms()
    _same(f"{tag} terms", terms, c.terms)                         # the reference's critics as plain functions
    _same(f"{tag} recombined terms", _recombine(c, terms), c.costs)
    assert np.array_equal(col > 0, c.terms[:, 3] >= 100000.0)
    for a, b in (("u1_opt", c.optimal_u1), ("u2_opt", c.optimal_u2)):
        err = hp.rel_err(out[a], b)
        assert err <= G.TOL, f"{tag} {a}: {err:.3e}"


@pytest.mark.parametrize("name", G.SINGLE)
def test_step(name):
    c = G.case(name)
    eng = _engine(c)
    try:
        _assert_step(c, eng, eng.step_injected(c.u1, c.u2, c.proj))
    finally:
        eng.close()


def test_chain3():
    """Three consecutive steps of the reference's run(): one engine, the state of every step set as
    the reference fed it back, the nominal sequence fed forward from the fixture's optimal_u*."""
    c0 = G.case(G.CHAIN[0])
    eng = _engine(c0)
    try:
        for name in G.CHAIN:
            c = G.case(name)
            eng.set_state(G.engine_state(c))
            eng.set_nominal(c.u_nom1, c.u_nom2)
            _assert_step(c, eng, eng.step_injected(c.u1, c.u2, c.proj))
    finally:
        eng.close()


@pytest.mark.parametrize("name", G.SINGLE)
def test_scorer(name):
    c = G.case(name)
    eng = _engine(c)
    try:
        wheels = (c.lw, c.rw)
        sc = eng.score_paths(c.traj, c.v, *wheels)
        _same(f"{name} scored costs", sc["cost"], c.costs)
        _same(f"{name} scored terms", sc["terms"], c.terms)
        if name in G.ALT:
            weights = [c.p.f(w) for w in WEIGHTS]
            t5 = np.concatenate([c.terms, c.alt_orientation[:, None]], 1)
            eng.set_critics(slope="wheels", w_orientation=W_ORIENTATION)
            got = eng.score_paths(c.traj, c.v, *wheels)
            _same(f"{name} scored costs, orientation", got["cost"], A.recombine(t5, weights, W_ORIENTATION))
            t5[:, 1] = c.alt_slope
            eng.set_critics(slope="body", w_orientation=0.0)
            got = eng.score_paths(c.traj, c.v, *wheels)
            _same(f"{name} scored slope, body", got["terms"][:, 1], c.alt_slope)
            _same(f"{name} scored costs, body", got["cost"], A.recombine(t5, weights, 0.0))
            eng.set_critics(slope="body", w_orientation=W_ORIENTATION)
            got = eng.score_paths(c.traj, c.v, *wheels)
            _same(f"{name} scored costs, body + orientation", got["cost"], A.recombine(t5, weights, W_ORIENTATION))
    finally:
        eng.close()


@pytest.mark.parametrize("name", G.STEPS)           # (the tail is the 3D rollout in a 2D step too)
def test_tail(name):
    c = G.case(name)
    p = c.p
    eng = _engine(c, filter_k=p.opt_filter_k, filter_a=p.opt_filter_a)
    try:
        eng.step_injected(np.tile(c.optimal_u1, (c.K, 1)), np.tile(c.optimal_u2, (c.K, 1)), "3d")
        d = eng.dump()
        for k in (0, c.K - 1):
            _same(f"{name} v", d["v"][k], c.v_opt)
            _same(f"{name} w", d["w"][k], c.w_opt)
            for a, b in (("traj", c.traj_sim), ("hv", c.hv_sim), ("lw", c.lw_sim), ("rw", c.rw_sim)):
                _same(f"{name} {a}", d[a][k], b)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ("chain3.1", "limits", "odd"))
def test_sampler_shifts_the_previous_optimum(name):
    """sigma 0: the sampled controls are the nominal sequence shifted by one, its last element kept
    (sampling_warp.py:71-92), clamped; the reference's u1 / u2 are that plus its noise."""
    c = G.case(name)
    assert c.u_nom1.any() and c.u_nom2.any()
    eng = _engine(c, state=G.engine_state(c, std_dev_u1=0.0, std_dev_u2=0.0))
    try:
        eng.set_nominal(c.u_nom1, c.u_nom2)
        eng.step(c.proj, 0)
        d = eng.dump()
        idx = np.minimum(np.arange(c.H) + 1, c.H - 1)
        for u, nom, lo, hi in ((d["u1"], c.u_nom1, "min_u1", "max_u1"), (d["u2"], c.u_nom2, "min_u2", "max_u2")):
            want = np.clip(nom[idx], c.p.f(lo), c.p.f(hi))
            assert not np.array_equal(want, np.clip(nom, c.p.f(lo), c.p.f(hi)))
            _same(f"{name} shifted", u, np.tile(want, (c.K, 1)))
        # and the reference's own samples are that sequence plus sigma times its noise, clamped
        e1, _ = G.noise(c)
        ref = np.clip(d["u1"] + F32(c.st.std_dev_u1) * e1, c.p.f("min_u1"), c.p.f("max_u1")).astype(F32)
        if name != "limits":                         # (clamped twice where the nominal sits on a bound)
            _same(f"{name} u1 from the engine's shifted sequence", ref, c.u1)
    finally:
        eng.close()
