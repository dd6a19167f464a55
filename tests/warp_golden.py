"""Loader of tests/golden/ref_warp_steps.npz: whole MPPI steps of the reference's own Warp kernels and
host class, run under oracle/warp_standin.py by tests/golden/make_warp_golden.py.
Shared by tests/test_reference_warp_oracle.py (CPU) and tests/test_gpu_reference_warp.py; it reads the
.npz alone."""
from __future__ import annotations

import functools
import json
import os
import types

import numpy as np

from oracle import mppi_ref as R

F32 = np.float32
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_warp_steps.npz")
CHAIN = ("chain3.0", "chain3.1", "chain3.2")
SINGLE = ("far3d", "far2d", "within_horizon", "near_goal", "collisions", "negative_quadrant", "reverse",
          "large_angle", "limits", "odd")
STEPS = SINGLE[:2] + CHAIN + SINGLE[2:]             # every step record under the "project" table
ALT = ("far3d", "within_horizon")
LIBM = ("collisions", "large_angle")
TOL = 1e-5                                          # BASELINE.json north_star, helpers.rel_err


class RefState(R.State):
    """The heading is the float32 vector the reference's kernels received, as it stands.  (Its run()
    feeds back a float32 heading and normalises it in float32; R.State normalises in float64, which
    can move the last bit of an already normalised float32 vector.)"""

    def heading_f32(self):
        return np.asarray(self.heading, F32)


@functools.lru_cache(maxsize=1)
def data():
    with np.load(PATH) as z:
        d = {k: z[k] for k in z.files}
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=1)
def scene():
    d = data()
    return R.Scene(d["Z"], float(d["half_width"]), d["costmap"])


@functools.lru_cache(maxsize=None)
def case(name):
    """One step record: its arrays as attributes, .meta, .cfg, .p (R.Params), .st (RefState), .proj."""
    d = data()
    pre = name + "/"
    c = types.SimpleNamespace(name=name, **{k[len(pre):]: v for k, v in d.items() if k.startswith(pre)})
    c.meta = json.loads(str(c.meta))
    c.cfg = cfg = c.meta["config"]
    c.proj = c.meta["proj"]
    c.K, c.H = cfg["K"], cfg["H"]
    c.p = R.Params(K=c.K, H=c.H, dt=cfg["dt"], robot_radius=cfg["robot_radius"], min_u1=cfg["min_u1"],
                   max_u1=cfg["max_u1"], min_u2=cfg["min_u2"], max_u2=cfg["max_u2"],
                   v_min_linear=cfg["min_linear_velocity"], v_max_linear=cfg["max_linear_velocity"],
                   v_min_angular=cfg["min_angular_velocity"], v_max_angular=cfg["max_angular_velocity"],
                   temperature=cfg["temperature"])
    s = c.meta["state"]
    c.st = RefState(x=s["x"], y=s["y"], heading=np.asarray(s["heading"], F32), left_wheel_speed=s["left_wheel_speed"],
                    right_wheel_speed=s["right_wheel_speed"], goal_x=s["goal_x"], goal_y=s["goal_y"],
                    std_dev_u1=s["std_dev_u1"], std_dev_u2=s["std_dev_u2"])
    return c


def params_kw(c, **over):
    """make_params' keywords of a case (the oracle's Params fields but K, H and seed)."""
    kw = {k: getattr(c.p, k) for k in ("dt", "robot_radius", "min_u1", "max_u1", "min_u2", "max_u2", "v_min_linear",
                                       "v_max_linear", "v_min_angular", "v_max_angular", "temperature")}
    kw.update(over)
    return kw


def engine_state(c, **over):
    """The engine's state of a case, with the heading's float32 components as the reference had them."""
    import dataclasses

    import helpers as hp
    st = dataclasses.replace(c.st, **over) if over else c.st
    s = hp.state_for(st)
    for i, h in enumerate(c.st.heading_f32()):
        s.heading[i] = float(h)
    return s


def noise(c):
    """(eps1, eps2) [K, H]: the table's values at the states the reference's sampler asked for, in the
    order it asked (per thread tid = k H + t: u1's state, then u2's)."""
    s = c.randn_states.reshape(c.K * c.H, 2)
    return c.randn_table[s[:, 0]].reshape(c.K, c.H), c.randn_table[s[:, 1]].reshape(c.K, c.H)
