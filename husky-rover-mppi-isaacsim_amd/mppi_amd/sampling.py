"""Sampling plans in numpy: the statement of DESIGN.md §4 D12 (include/mppi.h mppi_sampling).

A plan is dict(antithetic=, nominal=, beta=).  With z[k, t, c] the base normals of a step (Philox
key = seed, block step * ceil(H/2) + t/2, global trajectory k), the step's sampling normals e are,
all float32 and without contraction, in this order:

  correlation  beta > 0: e[0] = z[src(k), 0], e[t] = (beta e[t-1]) + (g z[src(k), t]), three roundings,
               g = float32(sqrt(1 - float64(beta)^2)); beta = 0: e = z
  antithetic   src(k) = k & ~1; an odd global k takes -e of k - 1 (an exact sign flip, both channels)
  nominal      global k = 0 gets +0.0 for every t and c (k = 1 then reflects its un-zeroed draw)

Usable without a GPU; the device's generator is csrc/mppi_detmath.h plan_source / plan_apply /
plan_ar1 and csrc/mppi_kernels.hip noise_gen / noise_serial.
"""
import math

import numpy as np

F32 = np.float32
SAMPLING_FIELDS = ("antithetic", "nominal", "beta")
DEFAULT_PLAN = dict(antithetic=False, nominal=False, beta=0.0)


def make_plan(antithetic=False, nominal=False, beta=0.0, k_offset=None):
    """A checked plan dict; ValueError names the field (the checks of mppi_set_sampling; the one on
    k_offset only where the caller knows it)."""
    for name, flag in (("antithetic", antithetic), ("nominal", nominal)):
        if not isinstance(flag, (bool, np.bool_)) and flag not in (0, 1):
            raise ValueError(f"{name} must be 0 or 1, got {flag!r}")
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"beta must be a number in [0, 1), got {beta!r}") from None
    if not (math.isfinite(b) and 0.0 <= float(F32(b)) < 1.0):
        raise ValueError(f"beta must be finite and in [0, 1), got {beta!r}")
    if antithetic and k_offset is not None and int(k_offset) & 1:
        raise ValueError(f"antithetic needs an even k_offset (a pair is global k, k + 1), got {k_offset}")
    return dict(antithetic=bool(antithetic), nominal=bool(nominal), beta=float(F32(b)))


def is_default(plan):
    p = make_plan(**plan)
    return not p["antithetic"] and not p["nominal"] and p["beta"] == 0.0


def plan_g(beta):
    """(float)sqrt(1.0 - (double)beta * (double)beta) of the float32 beta."""
    b = float(F32(beta))
    return F32(math.sqrt(1.0 - b * b))


def plan_sources(k, plan):
    """Global trajectory indices k -> (src, sign, zero): the trajectory whose base normals k reads,
    +1.0 / -1.0 (float32) and the mask of the rows that are all +0."""
    p = make_plan(**plan)
    k = np.atleast_1d(np.asarray(k, dtype=np.int64))
    src = (k & ~np.int64(1)) if p["antithetic"] else k.copy()
    sign = np.where((k & 1).astype(bool) & p["antithetic"], F32(-1.0), F32(1.0)).astype(F32)
    zero = (k == 0) & p["nominal"]
    return src, sign, zero


def correlate(z, beta):
    """The AR(1) recurrence along the last axis of z [n, H] (float32, three roundings per step)."""
    z = np.asarray(z, F32)
    b = F32(beta)
    if not b > 0:
        return z.copy()
    g = plan_g(b)
    e = np.empty_like(z)
    e[:, 0] = z[:, 0]
    for t in range(1, z.shape[1]):
        e[:, t] = (b * e[:, t - 1]).astype(F32) + (g * z[:, t]).astype(F32)
    return e


def apply_plan(z1, z2, k, plan):
    """The step's sampling normals (e1, e2) [n, H] of the global trajectories k, from the base normals
    z1, z2 [n, H] of their SOURCE trajectories plan_sources(k, plan)[0]."""
    p = make_plan(**plan)
    src, sign, zero = plan_sources(k, p)
    out = []
    for z in (z1, z2):
        z = np.asarray(z, F32)
        if z.ndim != 2 or z.shape[0] != src.size:
            raise ValueError(f"base normals must be [len(k), H], got {z.shape}")
        e = correlate(z, p["beta"])
        e = np.where(sign[:, None] < 0, -e, e).astype(F32)      # (an exact sign flip)
        e[zero] = F32(0.0)
        out.append(e)
    return out[0], out[1]
