"""GPU: the chain's transcendental-free reciprocal for near-unit norms (mppi_detmath.h recip_near1).

The reference normalises three vectors per rollout step that are unit already (the tangent a second
time, the rotated heading, the heading before the position update).  The chain forms the square root of
such a squared norm from its bit pattern and the reciprocal as 1 + (1 - b) (1 + 2^-13) in one fma: correctly
rounded for a squared norm within 2047 ulps of 1 (the guard), so every quotient stays the IEEE one.
  * the device self-test (what 6): every squared norm within 4096 ulps of 1 with 2^18 numerator triples
    each against sqrtf and a / b; every norm beyond 2047 ulps must come back flagged for the IEEE redo;
  * whole steps, bit for bit against the numpy restatement (oracle/), at the smallest shapes that reach
    every arm: K = 256 / 512 (one and two workgroups), H = 8 / 9 (odd H takes the peeled last step), on
    the role-split kernel, the pair kernel and the resident server, synchronous and with the deferred
    tail (tail_chain_3d runs the same helpers).  Scenes: C3; a flat DEM (every norm exactly 1, 1 - b = 0);
    the tilted plane (every lane on the IEEE redo) and the half plane (redo lanes beside fast lanes) of
    test_gpu_chain_ring.py; K = 256, H = 20 (the C1 shape) with seeds 0 - 2.
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
MODES = ("roles", "pair", "server")
TAILS = ("sync", "deferred-tail")
TINY = 2.0 ** -40
HALF_START = (-60.0, 0.0)


def test_device_selftest_near_unit_normalisation():
    st = hp.oracle_state()
    Z, hw, cm = hp.c3_scene()
    eng = hp.engine_for(64, 4, Z, hw, cm, st)
    try:
        for seed in (0, 1):
            bad = eng.selftest(6, n=8193 << 18, seed=seed)
            assert bad == 0, f"{bad} of 8193 * 2^18 items: a result differs from IEEE, or a norm beyond the guard came back unflagged"
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _scene(name):
    """c3: the C3 scene.  flat: its DEM replaced by zeros.  plane: by Z = float32(1e-14) * x.  half: only
    the rows of y < 0 replaced by the plane."""
    Z, hw, cm = hp.c3_scene()
    if name == "c3":
        return Z, hw, cm
    if name == "flat":
        return np.zeros_like(Z, dtype=np.float32), hw, cm
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
def _ref(scene, K, H, seed, start):
    """The oracle's step (computed once, shared by the modes and tails)."""
    Z, hw, cm = _scene(scene)
    st = hp.oracle_state(x=start[0], y=start[1])
    return R.mppi_step(R.Params(K=K, H=H, seed=seed), hp.oracle_scene(Z, hw, cm), st, np.zeros(H, np.float32),
                       np.zeros(H, np.float32), 0)


def _check(scene, K, H, seed, mode, tail, monkeypatch, start=hp.START):
    ref = _ref(scene, K, H, seed, start)
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
        eng.set_async_tail(tail == "deferred-tail")
        tag = f"{scene} K={K} H={H} seed={seed} {mode} {tail}"
        eng.step("3d", 0, copy=False)
        out = eng.outputs()
        for a, b in OUTS:
            assert np.array_equal(out[a], ref[b]), hp.mismatch_report(f"{tag} {a}", out[a], ref[b])
        info = eng.launch_info()
        if mode == "server":  # a shape that fell back to separate launches must not pass
            assert info["resident"] == 1 and info["server_steps"] == 1, info
            assert info["server_failed_steps"] == 0 and info["server_fallbacks"] == 0, info
        else:
            assert info["server_steps"] == 0, info
        costs = eng.costs()
        assert np.array_equal(costs, ref["cost"]), hp.mismatch_report(f"{tag} cost", costs, ref["cost"])
    finally:
        eng.close()


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,H", [(256, 8), (256, 9), (512, 8), (512, 9)])
def test_step_parity_c3(K, H, mode, tail, monkeypatch):
    _check("c3", K, H, 5, mode, tail, monkeypatch)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,H", [(256, 9), (512, 8)])
def test_step_parity_flat_dem(K, H, mode, tail, monkeypatch):
    """Every normal is (0, 0, 1) and every heading stays in the plane: the re-normalised vectors' norms
    are 1 or a few ulps from it, the reciprocal's 1 - b is 0 or a few ulps."""
    hv = _ref("flat", K, H, 5, hp.START)["parts"][0]["hv"]
    assert np.all(hv[..., 2] == 0), "the flat scene's headings leave the plane"
    _check("flat", K, H, 5, mode, tail, monkeypatch)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,H", [(256, 8), (512, 9)])
def test_step_parity_every_lane_on_the_ieee_redo(K, H, mode, tail, monkeypatch):
    hz = _ref("plane", K, H, 3, hp.START)["parts"][0]["hv"][..., 2]
    assert hz.shape == (K, H) and np.all(hz != 0) and np.all(np.abs(hz) < TINY), \
        "the scene does not put every lane on the redo at every step"
    _check("plane", K, H, 3, mode, tail, monkeypatch)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,H", [(256, 9), (512, 8)])
def test_step_parity_mixed_lanes_on_the_ieee_redo(K, H, mode, tail, monkeypatch):
    hz = _ref("half", K, H, 3, HALF_START)["parts"][0]["hv"][..., 2]
    trip = (np.abs(hz) < TINY).reshape(K // 64, 64, H).sum(axis=1)  # [wave, step] lanes below the guard
    assert np.all(((trip > 0) & (trip < 64)).any(axis=1)), f"a wave has no step with mixed lanes: {trip.tolist()}"
    _check("half", K, H, 3, mode, tail, monkeypatch, start=HALF_START)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_step_parity_c1_shape(seed, mode, tail, monkeypatch):
    _check("c3", 256, 20, seed, mode, tail, monkeypatch)
