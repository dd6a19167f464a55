"""CPU: the oracle (oracle/mppi_ref.py) against whole steps of the REFERENCE'S OWN Warp code.

tests/golden/ref_warp_steps.npz holds what the reference's kernels and its MPPI_Controller computed
when run under the project's Warp stand-in (tests/golden/make_warp_golden.py): the
launch order, the arguments and the resets are the reference's.  Every stage of the oracle is fed the
reference's inputs to that stage and must give the reference's outputs bit for bit, so a misreading
of a weight, a loop bound, an argument or the sampler's shift fails here instead of living in the
oracle and the kernels alike.

What is not bitwise, and why: the emitted controls of the oracle's whole step.  The oracle sums the
softmax in float64 in a fixed tree (D2), the reference in float32 in launch order; they are held to
the project's 1e-5 (BASELINE.json, helpers.rel_err).  The "libm" fixtures (float64 libm rounded once
instead of oracle.dmath) are held to that 1e-5 on the controls only; the relative difference of
their costs is measured by the generator and recorded in the fixture and in DESIGN.md §7.
"""
import importlib.util
import os

import numpy as np
import pytest

import alt_critics_refs as A
import helpers as hp
import warp_golden as G
from oracle import mppi_ref as R

F32 = np.float32


def _same(name, got, want):
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype == F32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), hp.mismatch_report(name, got, want)


# ------------------------------------------------------------------ the fixture itself
def test_fixture_is_what_the_issue_asked_for():
    d = G.data()
    assert os.path.getsize(G.PATH) < 1_000_000
    assert d["Z"].shape == (160, 160) and d["costmap"].shape == (20, 20) and d["Z"].dtype == F32
    assert 0.08 < np.mean(d["costmap"] > 0.99) < 0.12
    names = {k.split("/")[0] for k in d if "/" in k} - {"libm"}
    assert names == set(G.STEPS)
    for name in G.STEPS:
        c = G.case(name)
        assert c.meta["math"] == "project" and c.meta["settled_minimum"] is True
        assert c.K == (65 if name == "odd" else 64) and c.H <= 24
        assert c.u1.shape == (c.K, c.H) and c.traj.shape == (c.K, c.H, 3) and c.traj_sim.shape == (c.H, 3)
        assert np.array_equal(c.st.heading_f32(), np.asarray(c.meta["state"]["heading"], F32))
        assert abs(float(np.linalg.norm(c.st.heading_f32().astype(np.float64))) - 1.0) < 1e-6
    assert [G.case(n).meta["step"] for n in G.CHAIN] == [0, 1, 2]
    for name in G.LIBM:
        assert G.case("libm/" + name).meta["math"] == "libm"


# ------------------------------------------------------------------ stage by stage, bitwise
@pytest.mark.parametrize("name", G.STEPS)
def test_sampling_and_noise_placement(name):
    c = G.case(name)
    K, H, seed = c.K, c.H, c.meta["seed"]
    # sampling_warp.py:71-92: thread tid = k H + t asks for seed + tid + H and + 2H, the last element of
    # a sequence for + 3H and + 4H
    tid = np.arange(K * H)
    last = (tid % H) == H - 1
    want = np.stack([seed + tid + np.where(last, 3 * H, H), seed + tid + np.where(last, 4 * H, 2 * H)], 1)
    assert H + 1 <= seed < 1000                      # MPPI_isaac.py:517
    assert np.array_equal(c.randn_states.reshape(K * H, 2), want)
    e1, e2 = G.noise(c)
    u1, u2 = R.sample_controls(c.p, c.st, c.u_nom1, c.u_nom2, e1, e2)
    _same("u1", u1, c.u1)
    _same("u2", u2, c.u2)
    if c.meta["nominal"] or c.meta["step"] > 0:      # the shift by one is visible only off a zero nominal
        assert c.u_nom1.any() and c.u_nom2.any()
        unshifted = R.clampf(c.u_nom1[None, :] + F32(c.st.std_dev_u1) * e1, c.p.f("min_u1"), c.p.f("max_u1"))
        assert not np.array_equal(unshifted.astype(F32), c.u1)


@pytest.mark.parametrize("name", G.STEPS)
def test_wheel_filter(name):
    c = G.case(name)
    v, w = R.wheel_filter(c.p, c.st, c.u1, c.u2, c.p.filter_k, c.p.filter_a)
    _same("v", v, c.v)
    _same("w", w, c.w)


@pytest.mark.parametrize("name", G.STEPS)
def test_rollouts(name):
    c = G.case(name)
    roll = R.rollout3d if c.proj == "3d" else R.rollout2d
    traj, hv, lw, rw = roll(c.p, G.scene(), c.st, c.v, c.w)
    for n, got in (("traj", traj), ("hv", hv), ("lw", lw), ("rw", rw)):
        _same(n, got, getattr(c, n))


@pytest.mark.parametrize("name", G.STEPS)
def test_critics(name):
    c = G.case(name)
    _same("costs", R.critics(c.p, G.scene(), c.st, c.traj, c.lw, c.rw, c.v), c.costs)
    terms = np.stack(R.critic_terms(c.p, G.scene(), c.st, c.traj, c.lw, c.rw, c.v), -1)
    _same("terms", terms, c.terms)


@pytest.mark.parametrize("name", G.ALT)
def test_alternate_critics(name):
    """_avoid_slope and _path_orientation_critic, which the reference never launches: its functions
    were called on every rollout of the case; the alt-critic oracle gives those rows."""
    c = G.case(name)
    body = A.terms(c.p, G.scene(), c.st, c.traj, c.traj, c.traj, c.v)[:, 1]
    _same("alt_slope", body, c.alt_slope)
    _same("alt_orientation", A.orientation(c.st, c.traj), c.alt_orientation)
    assert not np.array_equal(c.alt_slope, c.terms[:, 1])          # the body path is not the wheels'


def test_alternate_critics_take_both_branches():
    po = np.concatenate([G.case(n).alt_orientation for n in G.ALT])
    assert (po != 0).sum() >= 8 and (po == 0).sum() >= 8


@pytest.mark.parametrize("name", G.STEPS)
def test_update(name):
    """weights, weights_sum and optimal_u* of the reference's float32 update in ascending thread order,
    after its reset("sim") (optimal_u* start from zero, not from the previous optimum)."""
    c = G.case(name)
    w, S = R.reference_weights_f32(c.costs, c.p.temperature)
    _same("weights", w, c.weights)
    _same("weights_sum", np.asarray([S]), c.weights_sum)
    o1, o2 = R.reference_update_f32(c.costs, c.u1, c.u2, c.p.temperature)
    _same("optimal_u1", o1, c.optimal_u1)
    _same("optimal_u2", o2, c.optimal_u2)
    assert c.weights.max() == 1.0 and c.weights_sum[0] >= 1.0


@pytest.mark.parametrize("name", G.STEPS)
def test_tail(name):
    c = G.case(name)
    # a root record [m, S, V1, V2] with S = 1 and V = the reference's optimal_u*: V / S is exact
    root = np.concatenate([[float(c.costs.min()), 1.0], c.optimal_u1, c.optimal_u2]).astype(np.float64)
    out = R.finish(c.p, G.scene(), c.st, root)
    _same("u1_opt", out["u1_opt"], c.optimal_u1)
    _same("u2_opt", out["u2_opt"], c.optimal_u2)
    for a, b in (("v_opt", "v_opt"), ("w_opt", "w_opt"), ("traj_sim", "traj_sim"), ("hv_sim", "hv_sim"),
                 ("lw_sim", "lw_sim"), ("rw_sim", "rw_sim")):
        _same(a, out[a], getattr(c, b))


# ------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("name", G.STEPS)
def test_whole_step(name):
    c = G.case(name)
    out = R.mppi_step(c.p, G.scene(), c.st, c.u_nom1, c.u_nom2, 0, proj=c.proj, injected=(c.u1, c.u2))
    _same("costs", out["cost"], c.costs)
    for a, b in (("u1_opt", c.optimal_u1), ("u2_opt", c.optimal_u2)):
        err = hp.rel_err(out[a], b)
        assert err <= G.TOL, f"{a}: {err:.3e}"


@pytest.mark.parametrize("name", G.LIBM)
def test_libm_table_controls(name):
    """The reference's step with float64 libm rounded once in place of oracle.dmath: the oracle's
    emitted controls stay within the project's 1e-5 of it.  The costs are not asserted (measured:
    the fixture's meta)."""
    c, lib = G.case(name), G.case("libm/" + name)
    assert "cost_rel_diff_from_project_max" in lib.meta
    out = R.mppi_step(c.p, G.scene(), c.st, c.u_nom1, c.u_nom2, 0, proj=c.proj, injected=(c.u1, c.u2))
    for a, b in (("u1_opt", lib.optimal_u1), ("u2_opt", lib.optimal_u2)):
        err = hp.rel_err(out[a], b)
        assert err <= G.TOL, f"{a}: {err:.3e}"


# ------------------------------------------------------------------ the fixture can be made again
def _generator():
    path = os.path.join(os.path.dirname(G.PATH), "make_warp_golden.py")
    spec = importlib.util.spec_from_file_location("make_warp_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_regenerating_far3d_gives_the_committed_file():
    gen = _generator()
    if not gen.reference_present():
        pytest.skip("the reference tree is not on this machine")
    entries = gen.case_entries("far3d", gen.make_case("far3d"))
    d = G.data()
    assert set(entries) == {k for k in d if k.startswith("far3d/")}
    for k, v in entries.items():
        v = np.asarray(v)
        assert v.dtype == d[k].dtype and np.array_equal(v, d[k]), k
    import sys
    assert "warp" not in sys.modules                 # the stand-in does not stay behind
