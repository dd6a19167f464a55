"""GPU: the critic set (mppi_set_critics: body-slope mode and the path-orientation critic) on the step
path, against the wrapped oracle (tests/alt_critics_refs.py).  Costs, emitted controls and the *_sim
arrays are bitwise the oracle's, on both rollout kernels."""
import ctypes as C

import numpy as np
import pytest

import alt_critics_refs as A
import helpers as hp
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT = (("u1_opt", "u1_opt"), ("u2_opt", "u2_opt"), ("lin_vel", "v_opt"), ("ang_vel", "w_opt"),
       ("traj_sim", "traj_sim"), ("heading_sim", "hv_sim"), ("left_wheel_sim", "lw_sim"),
       ("right_wheel_sim", "rw_sim"))
DUMPED = (("u1", "u1"), ("u2", "u2"), ("v", "v"), ("w", "w"), ("traj", "traj"), ("hv", "hv"), ("lw", "lw"),
          ("rw", "rw"))
BODY = dict(slope="body", w_orientation=0.0)
# (64, 3): no slope term; (65, 4), (257, 5): one; (1, 7), (130, 8), (513, 9): the wheel wave's 4-step A / B
# period on either side; (300, 24): ragged K; (256, 20): C1
BODY_SHAPES = [(64, 3), (65, 4), (257, 5), (1, 7), (130, 8), (513, 9), (300, 24), (256, 20)]


@pytest.fixture(params=["roles", "pair"])
def rollout_kernel(request, monkeypatch):
    """Both rollout kernels, forced by MPPI_ROLES, which a context reads when it is created."""
    monkeypatch.setenv("MPPI_ROLES", "1" if request.param == "roles" else "0")
    return request.param


def _weights(eng):
    p = eng.params
    return [p.w_path, p.w_slope, p.w_speed, p.w_obstacle]


def _step(monkeypatch, K, H, crit, proj="3d", seed=5, step=0, heading=(1.0, 0.0, 0.0), goal=hp.GOAL, set_it=True):
    """(oracle step under `crit`, engine outputs, engine, state)."""
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state(heading=heading, wl=0.3, wr=0.5, goal=goal)
    A.use(monkeypatch, **crit)
    u = np.zeros(H, F32)
    ref = R.mppi_step(R.Params(K=K, H=H, seed=seed), hp.oracle_scene(Z, hw, cm), st, u, u, step, proj=proj)
    eng = hp.engine_for(K, H, Z, hw, cm, st, seed=seed)
    if set_it:
        eng.set_critics(**crit)
        assert eng.critics() == dict(crit)
    return ref, eng.step(proj, step), eng, st


def _same_step(ref, out, eng, tag=""):
    costs = eng.costs()
    assert np.array_equal(costs.view(np.uint32), ref["cost"].view(np.uint32)), \
        tag + hp.mismatch_report("cost", costs, ref["cost"])
    for a, b in OUT:
        assert np.array_equal(out[a].view(np.uint32), np.asarray(ref[b], F32).view(np.uint32)), \
            tag + hp.mismatch_report(a, out[a], ref[b])


@pytest.mark.parametrize("proj", ["2d", "3d"])
@pytest.mark.parametrize("K,H", BODY_SHAPES)
def test_body_mode_matches_the_oracle(monkeypatch, rollout_kernel, K, H, proj):
    ref, out, eng, _ = _step(monkeypatch, K, H, BODY, proj)
    try:
        _same_step(ref, out, eng, f"{K}x{H} {proj}: ")
    finally:
        eng.close()


@pytest.mark.parametrize("proj", ["2d", "3d"])
def test_body_mode_goal_inside_the_horizon(monkeypatch, rollout_kernel, proj):
    goal = (-57.0, -4.0)
    p = R.Params(K=512, H=40)
    assert np.hypot(goal[0] - hp.START[0], goal[1] - hp.START[1]) < p.horizon_f32()   # the path-follow sum branch
    ref, out, eng, _ = _step(monkeypatch, 512, 40, BODY, proj, seed=6, goal=goal)
    try:
        _same_step(ref, out, eng)
    finally:
        eng.close()


@pytest.mark.parametrize("heading", [A.SIDE, A.BACK], ids=["side", "back"])
@pytest.mark.parametrize("K,H", [(65, 2), (256, 20), (513, 9)])
def test_orientation_matches_the_oracle(monkeypatch, rollout_kernel, K, H, heading):
    crit = dict(slope="wheels", w_orientation=1000.0)
    ref, out, eng, st = _step(monkeypatch, K, H, crit, heading=heading)
    try:
        po = A.orientation(st, ref["parts"][0]["traj"])
        if heading == A.BACK:
            assert (po != 0).all()                  # the term is in every cost
        elif H > 2:                                 # both branches are taken (two steps sideways never turn back)
            assert (po != 0).any() and (po == 0).any()
        _same_step(ref, out, eng)
    finally:
        eng.close()


@pytest.mark.parametrize("proj", ["2d", "3d"])
def test_body_and_orientation_together(monkeypatch, rollout_kernel, proj):
    crit = dict(slope="body", w_orientation=1000.0)
    ref, out, eng, _ = _step(monkeypatch, 300, 24, crit, proj, heading=A.SIDE, step=3)
    try:
        _same_step(ref, out, eng)
    finally:
        eng.close()


def test_defaults_keep_their_bits(monkeypatch, rollout_kernel):
    """A context that never called set_critics, one given {WHEELS, 0}, and the unwrapped oracle."""
    K, H = 300, 24
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state(wl=0.3, wr=0.5)
    u = np.zeros(H, F32)
    ref = R.mppi_step(R.Params(K=K, H=H, seed=5), hp.oracle_scene(Z, hw, cm), st, u, u, 3)
    never = hp.engine_for(K, H, Z, hw, cm, st, seed=5)
    given = hp.engine_for(K, H, Z, hw, cm, st, seed=5)
    try:
        assert never.critics() == A.DEFAULT
        given.set_critics("body", 7.0)
        given.set_critics("wheels", 0.0)
        _same_step(ref, never.step("3d", 3), never, "never set: ")
        _same_step(ref, given.step("3d", 3), given, "set to the defaults: ")
    finally:
        never.close()
        given.close()


@pytest.mark.parametrize("proj", ["2d", "3d"])
@pytest.mark.parametrize("crit", [A.DEFAULT, BODY, dict(slope="wheels", w_orientation=1000.0),
                                  dict(slope="body", w_orientation=1000.0)],
                         ids=["default", "body", "orientation", "body+orientation"])
def test_dump_score_and_terms(monkeypatch, rollout_kernel, crit, proj):
    K, H = 300, 24
    ref, out, eng, st = _step(monkeypatch, K, H, crit, proj, heading=A.SIDE, step=2)
    try:
        costs = eng.costs()
        d = eng.dump()
        part = ref["parts"][0]
        for name, key in DUMPED:      # body mode leaves the dumped wheel arrays what they are
            assert np.array_equal(d[name], part[key]), hp.mismatch_report(name, d[name], part[key])
        # score_paths on the dump, wheel arrays supplied in every mode
        sc = eng.score_paths(d["traj"], d["v"], d["lw"], d["rw"])
        assert np.array_equal(sc["cost"].view(np.uint32), costs.view(np.uint32)), \
            hp.mismatch_report("score_paths cost", sc["cost"], costs)
        t5, col5 = eng.cost_terms5()
        t4, col4 = eng.cost_terms()
        assert t5.shape == (K, 5) and t4.shape == (K, 4)
        assert np.array_equal(t5[:, :4].view(np.uint32), t4.view(np.uint32)) and np.array_equal(col4, col5)
        assert np.array_equal(t4.view(np.uint32), sc["terms"].view(np.uint32))
        assert np.array_equal(t5[:, 4].view(np.uint32), A.orientation(st, part["traj"]).view(np.uint32))
        c5 = A.recombine(t5, _weights(eng), crit["w_orientation"])
        assert np.array_equal(c5.view(np.uint32), costs.view(np.uint32)), hp.mismatch_report("terms5", c5, costs)
        if crit["w_orientation"] == 0:
            c4 = A.recombine(np.concatenate([t4, np.zeros((K, 1), F32)], 1), _weights(eng), 0.0)
            assert np.array_equal(c4.view(np.uint32), costs.view(np.uint32))
        if crit["slope"] == "body":   # term 1 is the slope value of the mode in force: the body path's
            body = eng.score_paths(d["traj"], d["v"])
            assert np.array_equal(body["terms"][:, 1].view(np.uint32), t4[:, 1].view(np.uint32))
    finally:
        eng.close()


def test_score_path_of_one_waypoint_has_no_orientation_term(monkeypatch):
    ref, out, eng, st = _step(monkeypatch, 64, 3, A.DEFAULT)
    try:
        d = eng.dump()
        one = np.ones(64, np.int32)
        a = eng.score_paths(d["traj"], d["v"], lengths=one)
        eng.set_critics("wheels", 1000.0)
        b = eng.score_paths(d["traj"], d["v"], lengths=one)
        assert np.array_equal(a["cost"].view(np.uint32), b["cost"].view(np.uint32))
    finally:
        eng.close()


def _server_run(resident, crits, monkeypatch):
    """Back-to-back steps, step i under crits[i] (a change stops the server; the next launch carries it)."""
    from mppi_amd import _lib
    monkeypatch.setenv("MPPI_ROLES", "1")
    Z, hw, cm = hp.c3_scene()
    eng = _lib.Engine(_lib.make_params(512, 20, seed=3), 0)
    outs = []
    try:
        eng.set_option("resident", resident)
        eng.set_option("resident_idle_us", 100000)
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        last = None
        for i, crit in enumerate(crits):
            if crit != last:
                eng.set_critics(**crit)
                last = crit
            eng.set_state(_lib.make_state(-60.0 + 0.9 * i, -5.0 - 0.4 * i, (0.1 * i, 1.0, 0.0), 0.2 * i, 0.1 * i,
                                          65.0 - 3.0 * i, 10.0 + 2.0 * i, 0.25 + 0.03 * i, 0.4 - 0.02 * i))
            eng.step("3d", i, copy=False)
            o = eng.outputs()
            outs.append({k: o[k].copy() for k, _ in OUT})
        info = eng.launch_info()
        costs = eng.costs().copy()
    finally:
        eng.close()
    return outs, costs, info


def test_server_steps_equal_separate_launches(monkeypatch):
    both = dict(slope="body", w_orientation=1000.0)
    for crits in ([both] * 4, [A.DEFAULT, A.DEFAULT, both, both]):
        g, gc, gi = _server_run(2, crits, monkeypatch)
        r, rc, ri = _server_run(0, crits, monkeypatch)
        assert ri["resident"] == 0 and ri["server_steps"] == 0, ri
        assert gi["resident"] == 1 and gi["server_steps"] == 4 and gi["server_failed_steps"] == 0, gi
        for i, (a, b) in enumerate(zip(g, r)):
            for k, _ in OUT:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (i, k)
        assert np.array_equal(gc.view(np.uint32), rc.view(np.uint32))
    # the set changed between steps 1 and 2 took effect: the same steps under the defaults differ
    d, dc, _ = _server_run(2, [A.DEFAULT] * 4, monkeypatch)
    assert all(np.array_equal(d[i]["u1_opt"], g[i]["u1_opt"]) for i in (0, 1))
    assert not np.array_equal(d[2]["u1_opt"], g[2]["u1_opt"])
    assert not np.array_equal(dc, gc)


def test_injected_controls_in_body_mode(monkeypatch, rollout_kernel):
    K, H = 300, 12
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state(wl=0.3, wr=0.5)
    rng = np.random.RandomState(0)
    u1 = rng.uniform(-1, 1, (K, H)).astype(F32)
    u2 = rng.uniform(-1, 1, (K, H)).astype(F32)
    A.use(monkeypatch, **BODY)
    u = np.zeros(H, F32)
    ref = R.mppi_step(R.Params(K=K, H=H), hp.oracle_scene(Z, hw, cm), st, u, u, 0, injected=(u1, u2))
    eng = hp.engine_for(K, H, Z, hw, cm, st)
    try:
        eng.set_critics(**BODY)
        _same_step(ref, eng.step_injected(u1, u2), eng)
    finally:
        eng.close()


def test_two_member_group_on_one_device(monkeypatch):
    from mppi_amd import _lib
    K, H = 1024, 12
    crit = dict(slope="body", w_orientation=1000.0)
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state(heading=A.SIDE, wl=0.3, wr=0.5)
    A.use(monkeypatch, **crit)
    u = np.zeros(H, F32)
    ref = R.mppi_step(R.Params(K=K, H=H, seed=42), hp.oracle_scene(Z, hw, cm), st, u, u, 1, world=2)
    g = _lib.Group(_lib.make_params(K, H, seed=42), [0, 0])
    try:
        g.set_dem(Z, hw)
        g.set_costmap(cm, hw)
        g.set_state(hp.state_for(st))
        g.set_critics(**crit)
        assert all(m.critics() == crit for m in g.members)
        out = g.step("3d", 1)
        assert np.array_equal(g.costs().view(np.uint32), ref["cost"].view(np.uint32))
        for a, b in OUT:
            assert np.array_equal(out[a].view(np.uint32), np.asarray(ref[b], F32).view(np.uint32)), a
    finally:
        g.close()


def test_bad_fields_are_refused_and_named():
    from mppi_amd import _lib
    lib = _lib.load_library()
    eng = _lib.Engine(_lib.make_params(64, 1), 0)
    two = _lib.Engine(_lib.make_params(256, 20), 0)
    batch = None
    try:
        for k, word in ((_lib.MppiCritics(2, 0.0), b"slope_mode"), (_lib.MppiCritics(-1, 0.0), b"slope_mode"),
                        (_lib.MppiCritics(0, float("nan")), b"w_orientation"),
                        (_lib.MppiCritics(1, float("inf")), b"w_orientation"),
                        (_lib.MppiCritics(0, 1.0), b"num_iterations")):
            assert lib.mppi_set_critics(eng.ctx, C.byref(k)) == -1
            assert word in lib.mppi_last_error(), (word, lib.mppi_last_error())
        assert eng.critics() == A.DEFAULT               # a refused set changes nothing
        eng.set_critics("body", 0.0)                    # H = 1 without the orientation term is fine
        Z, hw, cm = hp.c3_scene()
        two.set_dem(Z, hw)
        two.set_costmap(cm, hw)
        batch = _lib.Batch(two, 2)
        rows = (_lib.MppiCritics * 3)(_lib.MppiCritics(1, 0.0), _lib.MppiCritics(0, 5.0), _lib.MppiCritics(3, 0.0))
        assert lib.mppi_batch_set_variant_critics(batch.h, 3, rows) == -1
        assert b"row 2" in lib.mppi_last_error() and b"slope_mode" in lib.mppi_last_error()
        assert lib.mppi_batch_set_variant_critics(batch.h, 1025, rows) == -1
        assert lib.mppi_batch_set_variant_critics(batch.h, 2, rows) == 0
        assert lib.mppi_batch_set_variant_critics(batch.h, 0, None) == 0
    finally:
        if batch is not None:
            batch.close()
        eng.close()
        two.close()
