"""CPU: the host side of per-episode parameter variants and batch scoring (include/mppi.h
mppi_batch_variant, mppi_batch_set_variants, mppi_batch_set_episode_variant, mppi_batch_score;
DESIGN.md §3.7).  No device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mppi_amd import _lib
from mppi_amd import batch as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mppi.h")
NEW = ("mppi_batch_variant_default", "mppi_batch_set_variants", "mppi_batch_set_episode_variant", "mppi_batch_score")


def test_variant_struct_layout():
    assert C.sizeof(_lib.MppiBatchVariant) == 56
    assert _lib.MppiBatchVariant.proj.offset == 52
    names = [n for n, _ in _lib.MppiBatchVariant._fields_]
    assert names == list(MB.VARIANT_PARAM_FIELDS) + list(MB.VARIANT_POLICY_FIELDS) + ["proj"]
    # the header lists the same fields in the same order
    text = open(HEADER).read()
    body = re.search(r"typedef struct mppi_batch_variant \{(.*?)\} mppi_batch_variant;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for line in body.split(";") for n in re.sub(r"^\s*(float|int32_t)", "", line).split(",")
                if n.strip()]
    assert declared == names


def test_make_variant_defaults_and_overrides():
    p = _lib.make_params(256, 20)
    v = _lib.make_variant()
    for n in MB.VARIANT_PARAM_FIELDS:
        assert getattr(v, n) == getattr(p, n), n
    assert (v.sigma_base, v.sigma_div, v.proj) == (np.float32(0.4), 1.0, 3)
    v = _lib.make_variant("2d", temperature=3.0, sigma_div=3.0)
    assert (v.temperature, v.sigma_div, v.proj, v.w_path) == (3.0, 3.0, 2, p.w_path)
    with pytest.raises(ValueError):
        _lib.make_variant(dt=0.1)
    d = _lib.variant_as_dict(v)
    assert set(d) == set(MB.VARIANT_PARAM_FIELDS) | set(MB.VARIANT_POLICY_FIELDS) | {"proj"}
    w = _lib.make_variant(**d)
    assert bytes(w) == bytes(v)


def test_variant_params_overrides_exactly_the_listed_fields():
    base = {n: float(getattr(_lib.make_params(256, 20), n)) for n, _ in _lib.MppiParams._fields_
            if n not in ("reserved0",)}
    var = MB.variant_dict("2d", **{n: 1000.0 + i for i, n in enumerate(MB.VARIANT_PARAM_FIELDS)},
                          sigma_base=0.125, sigma_div=7.0)
    run_policy = dict(sigma_base=0.4, sigma_div=1.0, goal_tol=0.75, check_every=3)
    params, pol, proj = MB.variant_params(base, var, run_policy, "3d")
    assert set(params) == set(base)
    changed = {n for n in base if params[n] != base[n]}
    assert changed == set(MB.VARIANT_PARAM_FIELDS)
    for i, n in enumerate(MB.VARIANT_PARAM_FIELDS):
        assert params[n] == np.float32(1000.0 + i) and isinstance(params[n], np.float32)
    assert pol == dict(sigma_base=np.float32(0.125), sigma_div=np.float32(7.0), goal_tol=0.75, check_every=3)
    assert proj == "2d"
    assert base["w_path"] == float(_lib.make_params(256, 20).w_path)          # the inputs are not modified
    assert run_policy["sigma_div"] == 1.0
    # no variant: the context's params and the run's policy and projection
    params, pol, proj = MB.variant_params(base, None, run_policy, "3d")
    assert params == base and pol == run_policy and proj == "3d"
    # the default policy is run()'s
    assert MB.variant_params({}, None)[1] == MB.RUN_POLICY
    # the library's range checks
    for field, value in (("temperature", 0.0), ("sigma_div", 0.0), ("proj", 4)):
        with pytest.raises(ValueError):
            MB.variant_params(base, dict(var, **{field: value}))
    with pytest.raises(ValueError):
        MB.variant_params(base, dict(temperature=3.0))     # a variant gives every field
    with pytest.raises(ValueError):
        MB.variant_dict("3d", dt=0.1)


def test_variant_dict_defaults_are_the_library_defaults():
    v = _lib.make_variant()
    d = MB.variant_dict()
    for n in _lib.VARIANT_FIELDS:
        assert np.float32(d[n]) == getattr(v, n), n
    assert d["proj"] == "3d"


def test_new_entry_points_refuse_a_null_batch():
    lib = _lib.load_library()
    v = _lib.make_variant()
    pol = _lib.make_policy()
    sc = _lib.MppiPathScores()
    calls = {
        "mppi_batch_variant_default": lambda: lib.mppi_batch_variant_default(None, 3, C.byref(pol), C.byref(v)),
        "mppi_batch_set_variants": lambda: lib.mppi_batch_set_variants(None, 1, C.byref(v)),
        "mppi_batch_set_episode_variant": lambda: lib.mppi_batch_set_episode_variant(None, 0, -1),
        "mppi_batch_score": lambda: lib.mppi_batch_score(None, None, None, C.byref(sc), None),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() != 0, name
        assert b"null batch" in lib.mppi_last_error(), name


def test_header_exports_and_prototypes_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w\s\*]*?\b(mppi_\w+)\s*\(", text, flags=re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared and name in exported and name in _lib._PROTOS, name
    assert set(_lib._PROTOS) == declared
