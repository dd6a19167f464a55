"""CPU: the host side of the critic set (include/mppi.h mppi_critics, mppi_set_critics,
mppi_get_cost_terms5, mppi_batch_set_variant_critics) and the self-checks of the reference wrapper
(tests/alt_critics_refs.py): the conditions the GPU cases rely on.  No device is touched."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import alt_critics_refs as A
import helpers as hp
from mppi_amd import _lib
from mppi_amd import batch as MB
from oracle import mppi_ref as R

F32 = np.float32
NEW = ("mppi_set_critics", "mppi_get_critics", "mppi_get_cost_terms5", "mppi_batch_set_variant_critics")


def test_struct_enum_and_prototypes():
    assert C.sizeof(_lib.MppiCritics) == 8
    assert [n for n, _ in _lib.MppiCritics._fields_] == ["slope_mode", "w_orientation"]
    text = open(hp.__file__.replace("tests/helpers.py", "include/mppi.h")).read()
    assert re.search(r"typedef struct mppi_critics \{ int32_t slope_mode; float w_orientation; \} mppi_critics;", text)
    assert re.search(r"MPPI_SLOPE_WHEELS = 0, MPPI_SLOPE_BODY = 1", text)
    assert re.search(r"MPPI_TERM_ORIENTATION = 4", text)
    assert _lib.SLOPE_MODES == {"wheels": 0, "body": 1}
    assert _lib.COST_TERMS5 == _lib.COST_TERMS + ("orientation",)
    for name in NEW:
        assert name in _lib._PROTOS, name


def test_null_handles_are_refused():
    lib = _lib.load_library()
    k = _lib.MppiCritics(0, 0.0)
    t = (C.c_float * 5)()
    for name, call in (("mppi_set_critics", lambda: lib.mppi_set_critics(None, C.byref(k))),
                       ("mppi_get_critics", lambda: lib.mppi_get_critics(None, C.byref(k))),
                       ("mppi_get_cost_terms5", lambda: lib.mppi_get_cost_terms5(None, t, None)),
                       ("mppi_batch_set_variant_critics",
                        lambda: lib.mppi_batch_set_variant_critics(None, 1, C.byref(k)))):
        assert call() == -1, name          # MPPI_EINVAL
        assert b"null" in lib.mppi_last_error(), name


def test_make_critics_names_the_bad_field():
    k = _lib.make_critics("body", 2.5)
    assert (k.slope_mode, k.w_orientation) == (1, 2.5)
    assert _lib.critics_as_dict(k) == dict(slope="body", w_orientation=2.5)
    assert _lib.critics_as_dict(_lib.make_critics()) == A.DEFAULT
    with pytest.raises(ValueError, match="slope"):
        _lib.make_critics("tracks")
    with pytest.raises(ValueError, match="slope"):
        _lib.make_critics(2)
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="w_orientation"):
            _lib.make_critics("wheels", bad)


def test_variant_dict_split():
    base = MB.variant_dict("2d", w_slope=3.0)
    v, k = MB.split_variant(base)
    assert v == base and k is None                         # no critic key: the context's set
    v, k = MB.split_variant(dict(base, slope="body"))
    assert v == base and k == dict(slope="body", w_orientation=0.0)
    v, k = MB.split_variant(dict(base, w_orientation=1e5))
    assert v == base and k == dict(slope="wheels", w_orientation=1e5)
    assert "slope" not in base                             # the input is not modified
    # what is left is exactly a mppi_batch_variant, so the existing checks still apply to it
    assert bytes(_lib.make_variant(**v)) == bytes(_lib.make_variant(**base))
    MB.variant_params({}, v)
    with pytest.raises(ValueError, match="slope"):
        MB.split_variant(dict(base, slope="tracks"))
    with pytest.raises(ValueError, match="w_orientation"):
        MB.split_variant(dict(base, w_orientation=float("nan")))


# ---- the reference wrapper's self-checks ----

@functools.lru_cache(maxsize=None)
def _single(proj, slope, wo, heading=(1.0, 0.0, 0.0)):
    return A.single_step(proj, dict(slope=slope, w_orientation=wo), heading)


@functools.lru_cache(maxsize=None)
def _loop(proj, slope, wo, heading=(1.0, 0.0, 0.0)):
    return A.loop(proj, dict(slope=slope, w_orientation=wo), heading)


def test_default_wrapper_is_the_oracle():
    ref, st = _single("3d", "wheels", 0.0)
    p = R.Params(K=A.K1, H=A.H1, seed=A.SEED1)
    plain = R.mppi_step(p, hp.oracle_scene(*hp.c3_scene()), st, np.zeros(A.H1, F32), np.zeros(A.H1, F32), 0)
    assert np.array_equal(ref["cost"].view(np.uint32), plain["cost"].view(np.uint32))
    # the one-hot terms recombine to the oracle's cost: the wrapper's summation is the oracle's
    part = plain["parts"][0]
    t = A.terms(p, hp.oracle_scene(*hp.c3_scene()), st, part["traj"], part["lw"], part["rw"], part["v"])
    t5 = np.concatenate([t, np.zeros((A.K1, 1), F32)], 1)
    c = A.recombine(t5, [p.f(w) for w in A.WEIGHTS], 0.0)
    assert np.array_equal(c.view(np.uint32), plain["cost"].view(np.uint32))


@pytest.mark.parametrize("proj", ["2d", "3d"])
def test_body_mode_changes_every_cost_and_control(proj):
    a, _ = _single(proj, "wheels", 0.0)
    b, _ = _single(proj, "body", 0.0)
    assert int((a["cost"] != b["cost"]).sum()) == A.K1
    assert int((a["u1_opt"] != b["u1_opt"]).sum()) == A.H1


def test_orientation_branches_of_the_single_step_case():
    counts = {}
    for h in (A.SIDE, A.BACK, (1.0, 0.0, 0.0)):
        ref, st = _single("3d", "wheels", 0.0, h)
        counts[h] = int((A.orientation(st, ref["parts"][0]["traj"]) != 0).sum())
    assert counts == {A.SIDE: 104, A.BACK: 256, (1.0, 0.0, 0.0): 0}
    # with every po == 0 the term adds +0: the same costs as without it
    a, _ = _single("3d", "wheels", 0.0)
    b, _ = _single("3d", "wheels", 1000.0)
    assert np.array_equal(a["cost"], b["cost"])
    a, _ = _single("3d", "wheels", 0.0, A.BACK)
    b, _ = _single("3d", "wheels", 1000.0, A.BACK)
    assert int((a["cost"] != b["cost"]).sum()) == A.K1


def test_orientation_zero_denominator_is_defined():
    st = hp.oracle_state(x=3.0, y=4.0, goal=(3.0, 4.0))
    traj = np.zeros((2, 2, 3), F32)
    traj[:, 1, 0] = (1.0, -1.0)
    assert not A.orientation(st, traj).any()


@pytest.mark.parametrize("proj", ["2d", "3d"])
def test_closed_loop_body_changes_every_row(proj):
    assert A.rows_changed(_loop(proj, "wheels", 0.0), _loop(proj, "body", 0.0)) == A.STEPS_LOOP


def test_closed_loop_orientation_needs_a_large_weight():
    base = _loop("3d", "wheels", 0.0, A.BACK)
    assert base["steps"] == A.STEPS_LOOP
    assert A.rows_changed(base, _loop("3d", "wheels", 1000.0, A.BACK)) == 0
    assert A.rows_changed(base, _loop("3d", "wheels", 1e5, A.BACK)) == 5
