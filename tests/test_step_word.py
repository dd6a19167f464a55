"""CPU: the Python layer's side of the 64-bit sampling key, no library call.

A step outside [0, 2^64) is a ValueError in Engine.step, step_partial and Group.step before the C
function is reached (ctypes would reduce it modulo 2^64 in silence); every step inside arrives as it
is.  A seed is taken modulo 2^64 by make_params and make_task.  The oracle's noise wraps the block
index as the C arithmetic does.  The case list of tests/test_gpu_wide_key.py covers what it says.
"""
import ctypes as C

import numpy as np
import pytest

import wide_key_cases as WK
from mppi_amd import _lib
from oracle import dmath

TOP = 2 ** 64 - 1
GOOD = (0, 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, TOP, np.uint64(TOP), np.int64(7), True)
BAD = (-1, -2 ** 63, 2 ** 64, 2 ** 64 + 5, np.int64(-1))


class _Calls:
    """Stands in for the library: records the step word each entry point was called with."""

    def __init__(self):
        self.seen = []

    def _record(self, *args):
        self.seen.append(args[2])
        return 0

    mppi_step = mppi_step_partial = mppi_group_step = _record


def _engine(lib):
    eng = object.__new__(_lib.Engine)
    eng.lib, eng.ctx, eng._step_fn, eng._outref, eng._out = lib, C.c_void_p(1), lib.mppi_step, None, _lib.MppiOutputs()
    eng._owned = False            # (nothing to destroy)
    return eng


def _group(lib):
    g = object.__new__(_lib.Group)
    g.lib, g.h, g.members = lib, C.c_void_p(0), [_engine(lib)]
    return g


@pytest.mark.parametrize("step", GOOD, ids=str)
def test_a_step_inside_the_word_arrives_as_it_is(step):
    assert _lib.step_word(step) == int(step) and type(_lib.step_word(step)) is int
    lib = _Calls()
    _engine(lib).step("3d", step, copy=False)
    _engine(lib).step_partial(0x1000, "3d", step)
    _group(lib).step("3d", step, copy=False)
    assert lib.seen == [int(step)] * 3
    assert C.c_uint64(lib.seen[0]).value == int(step)


@pytest.mark.parametrize("step", BAD, ids=str)
def test_a_step_outside_the_word_is_refused_before_the_call(step):
    lib = _Calls()
    with pytest.raises(ValueError, match=r"step must lie in \[0, 2\^64\)"):
        _lib.step_word(step)
    with pytest.raises(ValueError, match="step must lie"):
        _engine(lib).step("3d", step)
    with pytest.raises(ValueError, match="step must lie"):
        _engine(lib).step_partial(0x1000, "3d", step)
    with pytest.raises(ValueError, match="step must lie"):
        _group(lib).step("3d", step)
    assert lib.seen == []


def test_seeds_are_taken_modulo_2_64():
    assert _lib.make_params(256, 5, seed=-1).seed == TOP
    assert _lib.make_params(256, 5, seed=2 ** 64 + 3).seed == 3
    assert _lib.make_params(256, 5, seed=0x9E3779B97F4A7C15).seed == 0x9E3779B97F4A7C15
    assert _lib.make_task(_lib.make_state(0.0, 0.0), -1, 3).seed == TOP
    assert _lib.make_task(_lib.make_state(0.0, 0.0), -2 ** 63, 3).seed == 2 ** 63


def test_oracle_noise_wraps_at_2_64():
    k = np.array([0, 5, 2 ** 32 + 3], np.int64)
    for a, b in ((2 ** 64, 0), (2 ** 64 + 9, 9)):            # the step after 2^64 - 1 is step 0
        for x, y in zip(dmath.noise(42, a, k, 5), dmath.noise(42, b, k, 5)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for x, y in zip(dmath.noise(-1, 3, k, 5), dmath.noise(TOP, 3, k, 5)):   # seed -1 is seed 2^64 - 1
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # (2^64 - 1) * 3 + 2 wraps inside the step: its last block is block 2^64 - 1 of the counter
    z = dmath.noise(42, TOP, k, 5)
    b = dmath.noise_block(42, TOP, k)
    assert np.array_equal(z[0][:, 4].view(np.uint32), b[0].view(np.uint32))
    assert not np.array_equal(z[0], dmath.noise(42, 2 ** 32 - 1, k, 5)[0])


def test_the_wide_key_cases_cover_every_value_with_every_form():
    """seed x plan and (k_offset = 2^32 - 100) x plan in full; every seed, k_offset and step with each of
    the three kernels launch_noise picks; one case at least with all three words wide per kernel."""
    cases = WK.CASES
    assert len(set(cases)) == len(cases)
    assert {(c[0], c[1]) for c in cases} >= {(pl, s) for pl in WK.PLANS for s in WK.SEEDS}
    assert {(c[0], c[2]) for c in cases} >= {(pl, WK.K_OFFSETS[0]) for pl in WK.PLANS}
    assert {WK.form(pl) for pl in WK.PLANS} == set(WK.FORMS)
    for i, values in ((1, WK.SEEDS), (2, WK.K_OFFSETS), (3, WK.STEPS)):
        assert {(WK.form(c[0]), c[i]) for c in cases} >= {(f, v) for f in WK.FORMS for v in values}
    wide = {WK.form(c[0]) for c in cases if (c[1] & WK.M64) >> 32 and c[2] >> 32 and c[3] >> 32}
    assert wide == set(WK.FORMS)
    assert all(c[2] % 2 == 0 for c in cases if WK.PLANS[c[0]]["antithetic"])     # (an odd k_offset refuses the plan)
