"""GPU: sampling plans on a context and a group (include/mppi.h mppi_sampling).

Everything is bitwise.  The expected step of a plan is the oracle's step on injected controls built
by the numpy statement (tests/sampling_refs.py).  Shapes: K = 300 (two ragged leaves) with H = 5 (odd:
the last Philox block half used, the recurrence crossing block borders) and K = 256, H = 20 (C1, the
server's plan); three closed-loop steps, so that u_nom != 0 makes the nominal row matter.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as hp
import sampling_refs as SR
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
EINVAL = -1
ALL_KEYS = ("u1_opt", "u2_opt", "lin_vel", "ang_vel", "traj_sim", "heading_sim", "left_wheel_sim", "right_wheel_sim")


@functools.lru_cache(maxsize=None)
def _expected(name, K, H, seed, proj, n_steps=3):
    return SR.closed_loop(K, H, seed, SR.PLANS[name], n_steps, proj)


def _drive(eng, steps, proj, tag, first=0):
    """Step the engine through the expected closed loop from step `first`, comparing every step."""
    for i in range(first, len(steps)):
        st, _, _, want = steps[i]
        eng.set_state(hp.state_for(st))
        eng.step(proj, i, copy=False)
        SR.same_step(eng.outputs(), eng.costs(), want, f"{tag} step {i}")


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("K,H", SR.SHAPES)
@pytest.mark.parametrize("name,proj", [(n, "3d") for n in SR.PLANS] + [("combined", "2d")])
def test_step_equals_oracle(name, proj, K, H, seed):
    steps = _expected(name, K, H, seed, proj)
    eng = SR.engine(K, H, seed, SR.PLANS[name])
    try:
        assert eng.get_sampling() == dict(SR.PLANS[name], beta=float(F32(SR.PLANS[name]["beta"])))
        _drive(eng, steps, proj, f"{name} {proj} K={K} H={H} seed={seed}")
    finally:
        eng.close()


def test_plans_change_the_step():
    """(the plans are not silently ignored: each moves the costs of step 0 off the default plan's)"""
    base = SR.closed_loop(300, 5, 0, SR.DEFAULT, 1)[0][3]["cost"]
    for name in SR.PLANS:
        c = _expected(name, 300, 5, 0, "3d")[0][3]["cost"]
        assert not np.array_equal(c, base), name


def test_odd_k_keeps_the_last_even_draw():
    """K = 257: global k = 256 is an even trajectory without a partner at a leaf start; it keeps its own draw."""
    K, H, seed = 257, 5, 1
    steps = SR.closed_loop(K, H, seed, SR.NOM_ANTI, 2)
    eng = SR.engine(K, H, seed, SR.NOM_ANTI)
    try:
        _drive(eng, steps, "3d", "K=257")
        u1 = eng.dump()["u1"]
    finally:
        eng.close()
    p = R.Params(K=K, H=H, seed=seed)
    st, n1, n2, _ = steps[1]
    own1, _ = SR.controls(p, st, n1, n2, 1, SR.DEFAULT, k_begin=256, k_count=1)
    assert np.array_equal(u1[256].view(np.uint32), own1[0].view(np.uint32))


@pytest.mark.parametrize("K,H", SR.SHAPES)
def test_dump_equals_mirror(K, H):
    seed = 1
    steps = _expected("combined", K, H, seed, "3d")
    eng = SR.engine(K, H, seed, SR.ALL)
    try:
        _drive(eng, steps, "3d", "dump")
        d = eng.dump()
    finally:
        eng.close()
    st, n1, n2, want = steps[-1]
    assert np.any(n1 != 0) and np.any(n2 != 0)
    for k in ("u1", "u2"):
        assert np.array_equal(d[k].view(np.uint32), want[k].view(np.uint32)), hp.mismatch_report(k, d[k], want[k])
    # row 0: the clamped shifted nominal sequence, written out on its own
    p = R.Params(K=K, H=H, seed=seed)
    idx = np.minimum(np.arange(H) + 1, H - 1)
    assert np.array_equal(d["u1"][0], R.clampf(np.asarray(n1, F32)[idx], p.f("min_u1"), p.f("max_u1")))
    assert np.array_equal(d["u2"][0], R.clampf(np.asarray(n2, F32)[idx], p.f("min_u2"), p.f("max_u2")))
    # row 1: the reflection of row 0's un-zeroed draw
    from mppi_amd import sampling as S
    from oracle import dmath
    z1, z2 = dmath.noise(seed, len(steps) - 1, np.zeros(1, np.int64), H)
    m1, m2 = R.sample_controls(p, st, n1, n2, -S.correlate(z1, 0.7), -S.correlate(z2, 0.7))
    assert np.array_equal(d["u1"][1].view(np.uint32), m1[0].view(np.uint32))
    assert np.array_equal(d["u2"][1].view(np.uint32), m2[0].view(np.uint32))


def _schedule_run(K, H, plan, roles=None, resident=None, async_tail=False, n_steps=4, monkeypatch=None):
    if roles is not None:
        monkeypatch.setenv("MPPI_ROLES", str(roles))
    eng = SR.engine(K, H, 3)
    if roles is not None:
        monkeypatch.delenv("MPPI_ROLES")
    try:
        if resident is not None:
            eng.set_option("resident", resident)
        eng.set_async_tail(async_tail)
        eng.set_sampling(**plan)
        outs = []
        for i in range(n_steps):
            eng.set_state(hp.state_for(hp.oracle_state(x=-60.0 + 0.5 * i, y=-5.0 + 0.2 * i, wl=0.1 * i, wr=0.2 * i,
                                                       goal=SR.FAR)))
            eng.step("3d", i, copy=False)
            o = eng.outputs()
            outs.append({k: o[k].copy() for k in ALL_KEYS})
            outs[-1]["cost"] = eng.costs()
        return outs, eng.launch_info()
    finally:
        eng.close()


def _same_runs(got, ref, tag):
    for i, (a, b) in enumerate(zip(got, ref)):
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{tag} step {i} {k}"


@pytest.mark.parametrize("name", ["combined", "nom_anti"])
def test_schedule_invariance(name, monkeypatch):
    plan = SR.ALL if name == "combined" else SR.NOM_ANTI
    K, H = 256, 20
    ref, info = _schedule_run(K, H, plan, resident=0)
    assert info["server_steps"] == 0
    for kw in (dict(roles=0), dict(roles=1), dict(resident=2), dict(resident=2, async_tail=True),
               dict(resident=0, async_tail=True)):
        got, info = _schedule_run(K, H, plan, monkeypatch=monkeypatch, **kw)
        _same_runs(got, ref, f"{name} {kw}")
        if kw.get("resident") == 2:
            if name == "nom_anti":
                assert info["server_steps"] > 0 and info["server_failed_steps"] == 0, info
            else:   # beta > 0: the serial generator does not fit the server's shares, separate launches
                assert info["server_steps"] == 0 and info["resident"] == 0, info


def test_server_noise_phase_takes_the_plan():
    """K = 2048 (8 leaves): the server's own noise phase generates the normals of step + 2 (at one or two
    leaves the noise kernel does); five steps on the server equal five separate-launch steps."""
    ref, _ = _schedule_run(2048, 6, SR.NOM_ANTI, resident=0, n_steps=5)
    got, info = _schedule_run(2048, 6, SR.NOM_ANTI, resident=2, n_steps=5)
    assert info["server_steps"] > 0 and info["server_failed_steps"] == 0, info
    _same_runs(got, ref, "server noise phase")
    dflt, _ = _schedule_run(2048, 6, SR.DEFAULT, resident=2, n_steps=1)
    assert not np.array_equal(dflt[0]["cost"], got[0]["cost"])


@pytest.mark.parametrize("resident", [0, 2])
@pytest.mark.parametrize("plan", ["combined", "nom_anti"])          # (nom_anti stays on the server at resident 2)
@pytest.mark.parametrize("K,H", SR.SHAPES)
def test_switching_plans(K, H, plan, resident):
    seed = 0
    plan = SR.ALL if plan == "combined" else SR.NOM_ANTI
    plans = [SR.DEFAULT, SR.DEFAULT, plan, SR.DEFAULT]
    steps = SR.closed_loop(K, H, seed, None, 4, plans=plans)
    eng = SR.engine(K, H, seed)
    fresh = SR.engine(K, H, seed)
    try:
        eng.set_option("resident", resident)
        for i in range(4):
            if i == 2:
                eng.set_sampling(**plan)         # the normals of steps 2 and 3 were generated ahead: dropped
            if i == 3:
                eng.set_sampling()
            st, n1, n2, want = steps[i]
            eng.set_state(hp.state_for(st))
            eng.step("3d", i, copy=False)
            got = eng.outputs()
            SR.same_step(got, eng.costs(), want, f"switch step {i}")
        # step 3 of a never-touched context from the same nominal and state
        st, n1, n2, want = steps[3]
        fresh.set_nominal(n1, n2)
        fresh.set_state(hp.state_for(st))
        fresh.step("3d", 3, copy=False)
        other = fresh.outputs()
        for k in ALL_KEYS:
            assert np.array_equal(got[k].view(np.uint32), other[k].view(np.uint32)), k
        assert np.array_equal(eng.costs(), fresh.costs())
    finally:
        eng.close()
        fresh.close()


def test_explicit_default_plan_changes_no_bit():
    K, H, seed = 256, 20, 1
    a, b = SR.engine(K, H, seed), SR.engine(K, H, seed)
    try:
        a.set_sampling(antithetic=False, nominal=False, beta=0.0)
        st = hp.oracle_state(wl=0.3, wr=0.5, goal=SR.FAR)
        sc = hp.oracle_scene(*hp.c3_scene())
        u1 = u2 = np.zeros(H, F32)
        for i in range(3):
            oa, ob = a.step("3d", i), b.step("3d", i)
            for k in ALL_KEYS:
                assert np.array_equal(oa[k].view(np.uint32), ob[k].view(np.uint32)), (i, k)
            assert np.array_equal(a.costs(), b.costs())
            want = R.mppi_step(R.Params(K=K, H=H, seed=seed), sc, st, u1, u2, i)     # today's oracle step
            SR.same_step(oa, a.costs(), want, f"default step {i}")
            u1, u2 = want["u1_opt"], want["u2_opt"]
    finally:
        a.close()
        b.close()


def test_group_of_two_equals_one_context():
    from mppi_amd import _lib
    K, H, seed = 1024, 6, 2
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state(wl=0.3, wr=0.5, goal=SR.FAR)
    one = SR.engine(K, H, seed, SR.ALL)
    g = _lib.Group(_lib.make_params(K, H, seed=seed), [0, 0])
    try:
        g.set_dem(Z, hw)
        g.set_costmap(cm, hw)
        g.set_state(hp.state_for(st))
        g.set_sampling(**SR.ALL)
        assert all(m.get_sampling()["antithetic"] for m in g.members)
        for i in range(3):
            a, b = g.step("3d", i), one.step("3d", i)
            for k in ALL_KEYS:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (i, k)
            assert np.array_equal(g.costs(), one.costs())
    finally:
        g.close()
        one.close()


def test_refusals_name_the_field():
    from mppi_amd import _lib
    eng = SR.engine(256, 5, 0)
    odd = SR.engine(256, 5, 0, k_offset=1)
    try:
        def refused(e, plan, word):
            rc = e.lib.mppi_set_sampling(e.ctx, C.byref(_lib.MppiSampling(*plan)))
            msg = e.lib.mppi_last_error().decode()
            assert rc == EINVAL and word in msg, (plan, rc, msg)

        before = eng.get_sampling()
        for beta in (1.0, -0.1, float("nan"), float("inf")):
            refused(eng, (0, 0, beta), "beta")
        refused(eng, (2, 0, 0.0), "antithetic")
        refused(eng, (-1, 0, 0.0), "antithetic")
        refused(eng, (0, 3, 0.0), "nominal")
        assert eng.get_sampling() == before
        refused(odd, (1, 0, 0.0), "antithetic")
        with pytest.raises(ValueError, match="antithetic.*k_offset"):      # (the Python layer knows the offset)
            odd.set_sampling(antithetic=True)
        odd.set_sampling(nominal=True, beta=0.5)      # (the other devices need no even offset)
        # the batch's rows: the row is named too
        batch = _lib.Batch(eng, 2)
        try:
            rows = (_lib.MppiSampling * 3)(_lib.MppiSampling(1, 1, 0.5), _lib.MppiSampling(0, 0, 0.0),
                                           _lib.MppiSampling(0, 0, 1.5))
            rc = eng.lib.mppi_batch_set_variant_sampling(batch.h, 3, rows)
            msg = eng.lib.mppi_last_error().decode()
            assert rc == EINVAL and "row 2" in msg and "beta" in msg, (rc, msg)
            rows[2] = _lib.MppiSampling(0, 7, 0.0)
            rc = eng.lib.mppi_batch_set_variant_sampling(batch.h, 3, rows)
            msg = eng.lib.mppi_last_error().decode()
            assert rc == EINVAL and "row 2" in msg and "nominal" in msg, (rc, msg)
            assert eng.lib.mppi_batch_set_variant_sampling(batch.h, 2, rows) == 0
            with pytest.raises(ValueError, match="beta"):
                batch.set_variant_sampling([dict(beta=1.0)])
        finally:
            batch.close()
    finally:
        eng.close()
        odd.close()
