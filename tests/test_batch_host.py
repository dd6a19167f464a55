"""CPU: the host side of the batched closed-loop episodes (include/mppi.h mppi_batch_*).

The C-ABI's argument checks (no device is touched), the ctypes mirrors, and the advance rule
(mppi_amd.batch.advance_state) against values worked out by hand and against the oracle closed loop
of tests/batch_refs.py (reference A), where no engine is involved.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import batch_refs as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mppi.h")
F32 = np.float32
BATCH_FUNCTIONS = ("mppi_batch_create", "mppi_batch_destroy", "mppi_batch_set_episode", "mppi_batch_run",
                   "mppi_batch_get_episode", "mppi_batch_get_log", "mppi_batch_get_ms")
EINVAL = -1


def test_header_and_prototypes_carry_the_batch_functions():
    from mppi_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn in BATCH_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % fn, text), fn
        assert fn in _lib._PROTOS, fn
    assert "#define MPPI_ABI_VERSION 1" in text
    assert re.search(r"typedef struct mppi_loop_policy \{\s*float sigma_base, sigma_div, goal_tol;\s*"
                     r"int32_t check_every;", text)


def test_loop_policy_layout():
    from mppi_amd import _lib
    assert ctypes.sizeof(_lib.MppiLoopPolicy) == 16
    assert [f[0] for f in _lib.MppiLoopPolicy._fields_] == ["sigma_base", "sigma_div", "goal_tol", "check_every"]
    assert _lib.MppiLoopPolicy.check_every.offset == 12
    p = _lib.make_policy()
    assert (p.sigma_base, p.sigma_div, p.goal_tol, p.check_every) == (F32(0.4), 1.0, 0.5, 0)


@pytest.fixture(scope="module")
def lib():
    from mppi_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd", "csrc"), "-j8"], check=True)
    return _lib.load_library()


def test_null_and_out_of_range_arguments_are_refused(lib):
    """MPPI_EINVAL before any device is touched (there is none here): the checks that need no batch."""
    from mppi_amd import _lib
    h = ctypes.c_void_p()
    st = _lib.make_state(0.0, 0.0)
    pol = _lib.make_policy()
    # a pointer that is never dereferenced: the episode count is checked before the context is read
    fake_ctx = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    assert lib.mppi_batch_create(None, 4, ctypes.byref(h)) == EINVAL
    assert b"null" in lib.mppi_last_error()
    assert lib.mppi_batch_create(None, 4, None) == EINVAL
    for episodes in (0, -1, 4097):
        assert lib.mppi_batch_create(fake_ctx, episodes, ctypes.byref(h)) == EINVAL
        assert b"episodes" in lib.mppi_last_error()
        assert not h.value
    lib.mppi_batch_destroy(None)   # a no-op
    for e in (0, -1, 1 << 20):
        assert lib.mppi_batch_set_episode(None, e, ctypes.byref(st), 1) == EINVAL
        assert lib.mppi_batch_get_episode(None, e, None, None, None, None, None, None) == EINVAL
        assert lib.mppi_batch_get_log(None, e, 0, 0, None) == EINVAL
    assert b"null" in lib.mppi_last_error()
    assert lib.mppi_batch_run(None, 3, 1, ctypes.byref(pol)) == EINVAL
    assert lib.mppi_batch_get_ms(None, None) == EINVAL
    ms = ctypes.c_double()
    assert lib.mppi_batch_get_ms(None, ctypes.byref(ms)) == EINVAL


def test_advance_state_by_hand():
    """Values chosen so that every operation of the rule is exact or has a known float32 rounding."""
    from mppi_amd import batch
    st = batch.state_dict(1.0, 2.0, (1.0, 0.0, 0.0), 0.1, 0.2, goal_x=9.0, goal_y=-3.0, std_dev_u1=0.25, std_dev_u2=0.3)
    # heading (3, 0, 4): norm 5 exactly; w = 0.5, r = 1.5: ww = 0.25, half = 0.375, all exact
    new, row = batch.advance_state(st, (1.5, 2.25, 0.125), (3.0, 0.0, 4.0), 0.75, 0.5, 1.5, batch.RUN_POLICY)
    assert new["x"] == F32(1.5) and new["y"] == F32(2.25)
    np.testing.assert_array_equal(new["heading"], np.array([0.6, 0.0, 0.8], np.float64).astype(F32))
    assert new["left_wheel_speed"] == F32(0.375) and new["right_wheel_speed"] == F32(1.125)
    assert new["goal_x"] == F32(9.0) and new["goal_y"] == F32(-3.0)
    # max(0.4f, 0.4f - 0.25f) = 0.4f; 0.4f + 0.25f in float32
    assert new["std_dev_u1"] == F32(0.4)
    assert new["std_dev_u2"] == F32(F32(0.4) + F32(0.25))
    np.testing.assert_array_equal(row, np.array([1.5, 2.25, 0.125, F32(0.6), 0.0, F32(0.8), 0.75, 0.5], F32))
    for v in list(new.values()) + [row]:
        assert np.asarray(v).dtype == F32
    # the Isaac policy: ww = (w w) / 3 rounded to float32 once, after the float32 product
    new, _ = batch.advance_state(st, (0, 0, 0), (0, 1, 0), 0.0, -0.7, 1.2, batch.ISAAC_POLICY)
    ww = F32(F32(F32(-0.7) * F32(-0.7)) / F32(3.0))
    assert new["std_dev_u1"] == F32(0.25) and new["std_dev_u2"] == F32(F32(0.25) + ww)
    half = F32(F32(F32(-0.7) * F32(1.2)) / F32(2.0))
    assert new["left_wheel_speed"] == F32(F32(0.0) - half) and new["right_wheel_speed"] == F32(F32(0.0) + half)
    # heading components are rounded to float32 from the float64 quotient (not divided in float32)
    hv = np.array([0.3, -0.2, 0.1], F32)
    d = hv.astype(np.float64)
    want = (d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])).astype(F32)
    np.testing.assert_array_equal(batch.normalise_heading(hv), want)


def test_activity_test():
    from mppi_amd import batch
    st = batch.state_dict(-60.0, -5.0, goal_x=-59.6, goal_y=-4.8)
    assert not batch.is_active(st)                               # inside the tolerance on both axes
    assert batch.is_active(st, dict(batch.RUN_POLICY, goal_tol=0.3))
    assert batch.is_active(batch.state_dict(-60.0, -5.0, goal_x=-59.6, goal_y=-4.4))   # y alone outside
    assert not batch.is_active(batch.state_dict(0.0, 0.0, goal_x=0.5, goal_y=-0.5))    # |d| == tol: not >


def test_advance_state_follows_the_oracle_closed_loop():
    """Episode 0 of the main case on the oracle (reference A): advance_state applied to the oracle's
    own step outputs gives the bits of the reference loop's rows and states at every step, its
    heading equals State.heading_f32() of the raw row, and the loop ends by the goal test."""
    import dataclasses
    from helpers import c3_scene, oracle_scene
    from mppi_amd import batch
    from oracle import mppi_ref as R
    ref = B.oracle_main(0)
    assert 0 < ref["steps"] < 40 and ref["reached"]
    start, goal, seed, K = B.MAIN[0]
    H = 20
    p = dataclasses.replace(R.Params(), K=K, H=H, seed=seed)
    sc = oracle_scene(*c3_scene())
    st = batch.state_dict(start[0], start[1], (1.0, 0.0, 0.0), goal_x=goal[0], goal_y=goal[1])
    u1 = np.zeros(H, F32)
    u2 = np.zeros(H, F32)
    raw_heading = np.array([1.0, 0.0, 0.0])   # the oracle normalises the raw row itself (State.heading_f32)
    i = 0
    while i < 40 and batch.is_active(st):
        S = R.State(x=float(st["x"]), y=float(st["y"]), heading=raw_heading,
                    left_wheel_speed=float(st["left_wheel_speed"]), right_wheel_speed=float(st["right_wheel_speed"]),
                    goal_x=float(st["goal_x"]), goal_y=float(st["goal_y"]), std_dev_u1=float(st["std_dev_u1"]),
                    std_dev_u2=float(st["std_dev_u2"]))
        o = R.mppi_step(p, sc, S, u1, u2, i, "3d")
        u1, u2 = o["u1_opt"], o["u2_opt"]
        st, row = batch.advance_state(st, o["traj_sim"][0], o["hv_sim"][0], o["v_opt"][0], o["w_opt"][0],
                                      p.robot_radius)
        np.testing.assert_array_equal(row, ref["rows"][i], err_msg=f"step {i}")
        raw_heading = np.asarray(o["hv_sim"][0], np.float64)
        np.testing.assert_array_equal(st["heading"], R.State(x=0.0, y=0.0, heading=raw_heading).heading_f32(),
                                      err_msg=f"heading, step {i}")
        i += 1
    assert i == ref["steps"]
    final = np.array([st["x"], st["y"], *st["heading"], st["left_wheel_speed"], st["right_wheel_speed"],
                      st["goal_x"], st["goal_y"], st["std_dev_u1"], st["std_dev_u2"]], F32)
    np.testing.assert_array_equal(final, ref["final"])
    np.testing.assert_array_equal(u1, ref["u1"])
