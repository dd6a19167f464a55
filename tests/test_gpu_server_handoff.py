"""GPU: the resident server's hand-offs at the shapes where they take another path.

The command travels host -> head -> the other workgroups as tagged 8-byte slots (csrc/mppi_cmd.h);
the workgroup with the last ticket starts the finish without polling the record count.  None of it
touches arithmetic, so the server on every step ("resident" 2) equals the separate launches
("resident" 0) bit for bit: every output of every step, the costs, and the nominal sequence the
closed loop carries.
  K = 256    one record: the only workgroup is head, finish and phase 2 at once
  K = 768    three records (a padded, non-power-of-two tree)
  K = 2048   eight records: the noise kernel runs instead of the server's noise shares
  H = 7      odd H, a single Philox block pair per row end;  H = 24
Every step has its own robot state and goal, so a stale or mixed command changes the result.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = ("u1_opt", "u2_opt", "lin_vel", "ang_vel", "traj_sim", "heading_sim", "left_wheel_sim", "right_wheel_sim")
STEPS = 6


def _state(i):
    from mppi_amd import _lib
    return _lib.make_state(-60.0 + 0.9 * i, -5.0 - 0.4 * i, (1.0, 0.05 * i, 0.0), left_wheel_speed=0.2 * i,
                           right_wheel_speed=0.1 * i, goal_x=65.0 - 3.0 * i, goal_y=10.0 + 2.0 * i,
                           std_dev_u1=0.25 + 0.03 * i, std_dev_u2=0.4 - 0.02 * i)


def _run(K, H, resident, async_tail, projs=("3d",), step_ids=None, costs_every_step=False):
    """STEPS closed-loop steps; returns (outputs per step, costs, final nominal, launch info)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mppi_amd import _lib, scene
    eng = _lib.Engine(_lib.make_params(K, H), 0)
    try:
        eng.set_option("resident", resident)
        # (an idle limit far above this loop's host work between steps: back-to-back steps share a launch)
        eng.set_option("resident_idle_us", 100000)
        Z, hw, cm = scene.scene_c3()
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        eng.set_async_tail(async_tail)
        outs, costs = [], []
        for n, i in enumerate(step_ids if step_ids is not None else range(STEPS)):
            eng.set_state(_state(n))
            eng.step(projs[n % len(projs)], i, copy=False)
            o = eng.outputs()
            outs.append({k: o[k].copy() for k in ALL})
            if costs_every_step:  # (stops the server: the next step starts a fresh launch)
                costs.append(eng.costs().copy())
        costs.append(eng.costs().copy())
        nominal = [np.array(x, copy=True) for x in eng.get_nominal()]
        info = eng.launch_info()
    finally:
        eng.close()
    return outs, costs, nominal, info


def _check(got, ref, served, tag):
    (g, gc, gn, gi), (r, rc, rn, ri) = got, ref
    assert ri["resident"] == 0 and ri["server_steps"] == 0, ri
    # a shape that fell back to separate launches must not pass
    assert gi["resident"] == 1 and gi["server_steps"] == served and gi["server_failed_steps"] == 0, gi
    assert len(g) == len(r) == served
    for i, (a, b) in enumerate(zip(g, r)):
        for k in ALL:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"step {i} {k} {tag}")
    assert len(gc) == len(rc)
    for i, (a, b) in enumerate(zip(gc, rc)):
        np.testing.assert_array_equal(a, b, err_msg=f"costs {i} {tag}")
    for a, b in zip(gn, rn):
        np.testing.assert_array_equal(a, b, err_msg=f"nominal {tag}")
    # the steps differ from one another (or a repeated command would pass too)
    assert not np.array_equal(g[0]["u1_opt"], g[-1]["u1_opt"]) or not np.array_equal(g[0]["u2_opt"], g[-1]["u2_opt"])


@pytest.mark.parametrize("async_tail", [False, True], ids=["sync", "deferred-tail"])
@pytest.mark.parametrize("H", [7, 24])
@pytest.mark.parametrize("K", [256, 768, 2048])
def test_server_equals_separate_launches(K, H, async_tail):
    ref = _run(K, H, 0, async_tail)
    got = _run(K, H, 2, async_tail)
    _check(got, ref, STEPS, f"K={K} H={H} async={async_tail}")
    assert got[3]["server_launches"] == 1, got[3]  # back to back: one launch served them all


def test_projection_alternates():
    """3d / 2d / 3d ...: another kernel instantiation each step, so the server is stopped and
    launched again between steps (the stop slot, first_seq and a relay left by the launch before)."""
    ref = _run(768, 7, 0, True, projs=("3d", "2d"), costs_every_step=True)
    got = _run(768, 7, 2, True, projs=("3d", "2d"), costs_every_step=True)
    _check(got, ref, STEPS, "proj alternates")
    assert got[3]["server_launches"] == STEPS, got[3]


def test_step_counter_jump():
    """A step counter that jumps: the normals of the new step are in no slot, the server is
    stopped, and a fresh launch takes the next command."""
    ids = [0, 1, 2, 11, 12, 13]
    ref = _run(2048, 24, 0, True, step_ids=ids)
    got = _run(2048, 24, 2, True, step_ids=ids)
    _check(got, ref, STEPS, "step jump")
    ref = _run(768, 24, 0, False, step_ids=ids)
    got = _run(768, 24, 2, False, step_ids=ids)
    _check(got, ref, STEPS, "step jump, three records")
