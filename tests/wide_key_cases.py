"""The case list of tests/test_gpu_wide_key.py, kept apart from it so that the list's
coverage is checked on the CPU (tests/test_step_word.py) while the cases themselves need a GPU."""
from __future__ import annotations

import sampling_refs as SR

M64 = 0xFFFFFFFFFFFFFFFF
H = 5
GOLDEN = 0x9E3779B97F4A7C15
S0 = 2 ** 32 // 3                     # 1431655765: n = 0xFFFFFFFF, 0x100000000, 0x100000001 inside the step
PLANS = dict(default=SR.DEFAULT, anti=SR.ANTI, nominal=SR.NOMINAL, beta=SR.BETA, all=SR.ALL)
SEEDS = (GOLDEN, 2 ** 32, 2 ** 64 - 1, -1)                  # (-1: through make_params, the bits of 2^64 - 1)
K_OFFSETS = (2 ** 32 - 100, 2 ** 33 + 2, 2 ** 36)           # all even: the antithetic plans are allowed
STEPS = (S0, 2 ** 40 + 7, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)


def form(plan):
    """The noise kernel launch_noise (csrc/mppi_kernels.hip) picks for a plan, restated: the serial
    kernel for beta > 0, the plan kernel for an elementwise plan, else the plain kernel."""
    p = PLANS[plan]
    return "serial" if p["beta"] > 0 else "plan" if p["antithetic"] or p["nominal"] else "plain"


FORMS = ("plain", "plan", "serial")


def cases():
    """(plan, seed, k_offset, step): seed x plan and (k_offset = 2^32 - 100) x plan in full; every other
    k_offset and every step with each of the three generator forms; all three words wide with each form."""
    names = list(PLANS)
    out = [(pl, seed, 0, 1) for seed in SEEDS for pl in names]
    out += [(pl, 42, K_OFFSETS[0], 1) for pl in names]
    out += [(pl, 42, K_OFFSETS[1], 2) for pl in ("default", "nominal", "all")]
    out += [(pl, 42, K_OFFSETS[2], 2) for pl in ("default", "anti", "beta")]
    per_form = (("default", "anti", "beta"), ("default", "nominal", "all"))
    for i, step in enumerate(STEPS):
        out += [(pl, 42, 0, step) for pl in per_form[i % 2]]
    out += [(pl, GOLDEN, K_OFFSETS[0], S0) for pl in ("default", "anti", "all")]
    out += [("nominal", 2 ** 64 - 1, K_OFFSETS[2], 2 ** 64 - 1), ("beta", -1, K_OFFSETS[1], 2 ** 63),
            ("default", 2 ** 32, K_OFFSETS[1], 2 ** 40 + 7)]
    return out


CASES = cases()


def case_id(c):
    return f"{c[0]}-seed{c[1]:#x}-k{c[2]:#x}-step{c[3]:#x}"
