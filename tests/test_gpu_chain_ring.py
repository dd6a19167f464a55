"""GPU: the rollout chain's ring slot, waits and IEEE redo at the shapes where they turn.

The chain wave (chain_wave_3d) walks rings six steps deep two steps per
iteration: a running slot that wraps every third iteration, two peeled last steps (one when H is
odd), and waits on the cached progress counters once per two steps.  None of it touches
arithmetic, so every case equals the numpy restatement (oracle/) bit for bit: the costs, every
output, and the dumped rollouts, on the role-split kernel, the pair kernel and the resident server.
  H = 1 .. 8      shorter than the ring, equal to it (6), one and two past it
  H = 11 .. 14    the second wrap, odd and even
  H = 19          three wraps and an odd tail that leaves the slot off zero
  K = 300         a second, ragged workgroup
Chained server steps catch a slot or limit that does not restart with each step the server serves.
The two plane scenes put every lane, and then only some lanes of every wave, on the IEEE redo
(the heading's z component below the fast path's 2^-40 guard).
"""
import functools

import numpy as np
import pytest

import helpers as hp
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

OUTS = (("u1_opt", "u1_opt"), ("u2_opt", "u2_opt"), ("lin_vel", "v_opt"), ("ang_vel", "w_opt"),
        ("traj_sim", "traj_sim"), ("heading_sim", "hv_sim"), ("left_wheel_sim", "lw_sim"),
        ("right_wheel_sim", "rw_sim"))
DUMPS = ("traj", "hv", "lw", "rw", "v", "w")
MODES = ("roles", "pair", "server")
TINY = 2.0 ** -40


@functools.lru_cache(maxsize=None)
def _scene(name):
    """c3: the C3 scene.  plane: its DEM replaced by Z = float32(1e-14) * x.  half: only the rows
    of y < 0 replaced."""
    Z, hw, cm = hp.c3_scene()
    if name == "c3":
        return Z, hw, cm
    n = Z.shape[0]
    x = np.float32(-hw) + np.arange(Z.shape[1], dtype=np.float32) * np.float32(2.0 * hw / Z.shape[1])
    plane = np.broadcast_to(np.float32(1e-14) * x, Z.shape).astype(np.float32)
    Zp = np.array(Z, dtype=np.float32, copy=True)
    if name == "plane":
        Zp[:] = plane
    else:
        Zp[n // 2:] = plane[n // 2:]
    return Zp, hw, cm


@functools.lru_cache(maxsize=None)
def _ref(scene, K, H, seed, start, steps=1):
    """The oracle's chain of `steps` steps, the nominal sequence fed back (computed once, shared by the modes)."""
    Z, hw, cm = _scene(scene)
    st = hp.oracle_state(x=start[0], y=start[1])
    p = R.Params(K=K, H=H, seed=seed)
    sc = hp.oracle_scene(Z, hw, cm)
    u1n, u2n = np.zeros(H, np.float32), np.zeros(H, np.float32)
    refs = []
    for step in range(steps):
        ref = R.mppi_step(p, sc, st, u1n, u2n, step)
        refs.append(ref)
        u1n, u2n = ref["u1_opt"], ref["u2_opt"]
    return refs


def _check(scene, K, H, seed, mode, monkeypatch, start=hp.START, steps=1):
    refs = _ref(scene, K, H, seed, start, steps)
    Z, hw, cm = _scene(scene)
    st = hp.oracle_state(x=start[0], y=start[1])
    if mode == "server":
        monkeypatch.delenv("MPPI_ROLES", raising=False)
    else:
        monkeypatch.setenv("MPPI_ROLES", "1" if mode == "roles" else "0")
    eng = hp.engine_for(K, H, Z, hw, cm, st, seed=seed)
    try:
        if mode == "server":
            eng.set_option("resident", 2)
            eng.set_option("resident_idle_us", 100000)
        else:
            eng.set_option("resident", 0)
        tag = f"{scene} K={K} H={H} {mode}"
        for step, ref in enumerate(refs):
            eng.step("3d", step, copy=False)
            out = eng.outputs()
            for a, b in OUTS:
                assert np.array_equal(out[a], ref[b]), hp.mismatch_report(f"{tag} step {step} {a}", out[a], ref[b])
        info = eng.launch_info()
        if mode == "server":  # a shape that fell back to separate launches must not pass
            assert info["resident"] == 1 and info["server_steps"] == steps, info
            assert info["server_failed_steps"] == 0 and info["server_fallbacks"] == 0, info
        else:
            assert info["server_steps"] == 0, info
        costs = eng.costs()
        assert np.array_equal(costs, refs[-1]["cost"]), hp.mismatch_report(f"{tag} cost", costs, refs[-1]["cost"])
        d = eng.dump()
        part = refs[-1]["parts"][0]
        for name in DUMPS:
            assert np.array_equal(d[name], part[name]), hp.mismatch_report(f"{tag} dump {name}", d[name], part[name])
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,H", [(256, h) for h in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 19)] + [(300, 7), (300, 12)])
def test_horizons_around_the_ring_depth(K, H, mode, monkeypatch):
    _check("c3", K, H, 11, mode, monkeypatch)


@pytest.mark.parametrize("H", [7, 13])
def test_chained_server_steps(H, monkeypatch):
    _check("c3", 256, H, 7, "server", monkeypatch, steps=4)


@pytest.mark.parametrize("mode", MODES)
def test_every_lane_on_the_ieee_redo(mode, monkeypatch):
    K, H = 256, 8
    hz = _ref("plane", K, H, 3, hp.START)[0]["parts"][0]["hv"][..., 2]
    assert hz.shape == (K, H) and np.all(hz != 0) and np.all(np.abs(hz) < TINY), \
        "the scene does not put every lane on the redo at every step"
    _check("plane", K, H, 3, mode, monkeypatch)


@pytest.mark.parametrize("mode", MODES)
def test_mixed_lanes_on_the_ieee_redo(mode, monkeypatch):
    K, H, start = 256, 12, (-60.0, 0.0)
    hz = _ref("half", K, H, 3, start)[0]["parts"][0]["hv"][..., 2]
    trip = (np.abs(hz) < TINY).reshape(K // 64, 64, H).sum(axis=1)  # [wave, step] lanes below the guard
    assert np.all(((trip > 0) & (trip < 64)).any(axis=1)), f"a wave has no step with mixed lanes: {trip.tolist()}"
    _check("half", K, H, 3, mode, monkeypatch, start=start)
