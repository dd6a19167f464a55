"""GPU: per-episode parameter variants of the batched episodes (mppi_batch_set_variants /
mppi_batch_set_episode_variant).

Contract: every step of an episode that holds a variant is bitwise the mppi_step of a context created
with the batch context's params overridden by the variant, with the variant's projection and sigma
schedule.  References A and B are in tests/batch_variant_refs.py; K = 256, H = 20, the C3 scene.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V

pytestmark = pytest.mark.gpu

MPPI_EINVAL = -1


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _policy(pol=B.RUN, check_every=0):
    from mppi_amd import _lib
    return _lib.make_policy(check_every=check_every, **pol)


def _run(episodes, variants, runs, proj="3d", pol=B.RUN, check_every=0, raw=False):
    """episodes: [(start, goal, seed, variant index)]; variants: list of dicts, or callables taking the
    batch (for Batch.variant_default); runs: step caps of successive runs.  raw: set the episodes
    through mppi_batch_set_episode alone, touching none of the variant entry points.  Returns per
    episode the result after the last run with the log rows of all runs concatenated."""
    _gpu()
    from mppi_amd import _lib
    eng = V.make_engine()
    try:
        batch = _lib.Batch(eng, len(episodes))
        if variants:
            batch.set_variants([v(batch) if callable(v) else v for v in variants])
        for e, (start, goal, seed, vi) in enumerate(episodes):
            st = V.mppi_state(B.start_state(start, goal))
            if raw:
                assert vi == -1
                assert eng.lib.mppi_batch_set_episode(batch.h, e, C.byref(st), seed) == 0
            else:
                batch.set_episode(e, st, seed, vi)
        logs = [[] for _ in episodes]
        for n in runs:
            batch.run(n, proj, _policy(pol, check_every))
            for e in range(len(episodes)):
                logs[e].append(batch.log(e))
        out = []
        for e in range(len(episodes)):
            r = V.collect(batch, e)
            r["rows"] = np.concatenate(logs[e])
            r["steps"] = len(r["rows"])
            assert r["total"] == r["steps"], (e, r["total"], r["steps"])
            out.append(r)
        batch.close()
    finally:
        eng.close()
    return out


MAIN_NAMES = list(V.VARIANTS) + ["default", "default_variant", "default_collision"]


@functools.lru_cache(maxsize=None)
def _main_case():
    names = list(V.VARIANTS)
    variants = [V.variant(n) for n in names] + [lambda b: b.variant_default("3d", _policy())]
    eps = [(V.VARIANTS[n][2], V.FAR, V.SEED, i) for i, n in enumerate(names)]
    eps += [(B.START, V.FAR, V.SEED, -1), (B.START, V.FAR, V.SEED, len(names)),
            (V.COLLISION_START, V.FAR, V.SEED, -1)]
    return dict(zip(MAIN_NAMES, _run(eps, variants, (V.CAP,))))


@pytest.mark.parametrize("name", MAIN_NAMES)
def test_main_case_matches_references(name):
    """One batch, one episode per variant of the issue plus an episode without a variant and one with
    variant_default, run with proj = 3d, cap 8: each is bitwise reference A (oracle loop) and
    reference B (fresh engine with the overridden params)."""
    got = _main_case()[name]
    ref_name = "default" if name == "default_variant" else name
    a = V.ref_a_named(ref_name)
    V.same(got, a, f"{name} vs A")
    if ref_name in V.VARIANTS:
        b = V.ref_b(V.VARIANTS[ref_name][2], V.FAR, V.SEED, V.CAP, V.variant(ref_name))
    else:
        b = V.ref_b(V.COLLISION_START if ref_name == "default_collision" else B.START, V.FAR, V.SEED, V.CAP, None)
    V.same(got, b, f"{name} vs B")
    assert got["steps"] == V.CAP and not got["reached"]


def test_main_case_variants_change_the_loop():
    """The default-variant episode equals the episode without a variant; every other variant changes at
    least one log row against the episode without a variant from the same start (so the inputs
    cannot go stale: a variant that is ignored fails test_main_case_matches_references)."""
    got = _main_case()
    V.same(got["default_variant"], got["default"], "variant_default vs no variant")
    for name in V.VARIANTS:
        base = got["default_collision" if name == "collision" else "default"]
        n = V.differ(got[name], base)
        print(f"{name}: {n} of {V.CAP} rows differ from the default 3D run")
        assert n >= 1, name


def test_mixed_projections_and_termination():
    """The five episodes of batch_refs.MAIN twice in one batch, under a 2D and under a 3D variant, cap 40:
    each equals its single-projection batch (pinned to the oracle by tests/test_gpu_batch.py), the
    episode that starts inside the tolerance (0 steps) and the one that runs to the cap included."""
    main = [(start, goal, seed, -1) for start, goal, seed, _ in B.MAIN]
    ref = {pj: _run(main, None, (40,), proj=pj, raw=True) for pj in ("2d", "3d")}
    variants = [lambda b: b.variant_default("2d", _policy()), lambda b: b.variant_default("3d", _policy())]
    eps = [(s, g, sd, 0) for s, g, sd, _ in main] + [(s, g, sd, 1) for s, g, sd, _ in main]
    # the run's own projection is ignored by episodes that hold a variant
    got = _run(eps, variants, (40,), proj="2d")
    for i in range(5):
        V.same(got[i], ref["2d"][i], f"episode {i} under the 2D variant")
        V.same(got[5 + i], ref["3d"][i], f"episode {i} under the 3D variant")
    for r in (got, ref["2d"], ref["3d"]):
        assert r[3]["steps"] == 0 and r[3]["reached"]
        assert r[4]["steps"] == 40 and not r[4]["reached"]
    assert V.differ(got[4], got[9]) >= 1   # the projections do differ


def test_neighbours_do_not_leak():
    """Identical start and seed, two variants interleaved v0, v1, v0, v1, ...: equal variants give equal
    results, different ones differ."""
    variants = [V.variant("temperature3"), V.variant("weights")]
    eps = [(B.START, V.FAR, V.SEED, e % 2) for e in range(8)]
    got = _run(eps, variants, (V.CAP,))
    for e in range(2, 8):
        V.same(got[e], got[e % 2], f"episode {e} vs episode {e % 2}")
    assert V.differ(got[0], got[1]) >= 1
    V.same(got[0], V.ref_a_named("temperature3"), "v0 vs A")
    V.same(got[1], V.ref_a_named("weights"), "v1 vs A")


@pytest.mark.parametrize("check_every", [1, 16])
def test_no_variants_gives_the_same_bits(check_every):
    """A batch that never calls the variant entry points equals one whose episodes all hold
    variant_default, across a split run (8 + 8 steps)."""
    main = [(start, goal, seed, -1) for start, goal, seed, _ in B.MAIN]
    plain = _run(main, None, (8, 8), check_every=check_every, raw=True)
    held = _run([(s, g, sd, 0) for s, g, sd, _ in main], [lambda b: b.variant_default("3d", _policy())], (8, 8),
                check_every=check_every)
    for e in range(len(main)):
        V.same(held[e], plain[e], f"episode {e}, check_every {check_every}")
    assert plain[4]["steps"] == 16
    assert len({r["steps"] for r in plain}) >= 3


def test_argument_checks():
    """Refused calls return MPPI_EINVAL and leave the batch as it was: it runs normally afterwards."""
    _gpu()
    from mppi_amd import _lib
    eng = V.make_engine()
    try:
        lib = eng.lib
        batch = _lib.Batch(eng, 2)
        good = [_lib.make_variant(**V.variant("temperature3")), _lib.make_variant(**V.variant("proj2d"))]

        def set_variants(rows, n=None):
            arr = (_lib.MppiBatchVariant * max(len(rows), 1))(*rows)
            return lib.mppi_batch_set_variants(batch.h, len(rows) if n is None else n, arr)

        def bad(**kw):
            v = _lib.make_variant(**V.variant("temperature3"))
            for k, x in kw.items():
                setattr(v, k, x)
            return v

        assert set_variants(good) == 0
        for e in range(2):
            batch.set_episode(e, V.mppi_state(B.start_state(B.START, V.FAR)), V.SEED, e)
        for index in (2, -2, 1024):
            assert lib.mppi_batch_set_episode_variant(batch.h, 0, index) == MPPI_EINVAL
            assert b"variant" in lib.mppi_last_error()
        assert lib.mppi_batch_set_episode_variant(batch.h, 2, 0) == MPPI_EINVAL      # no such episode
        assert set_variants(good[:1]) == MPPI_EINVAL                                  # episode 1 holds row 1
        assert b"episode 1" in lib.mppi_last_error()
        assert set_variants([]) == MPPI_EINVAL
        for field, value in (("temperature", 0.0), ("temperature", -1.0), ("temperature", float("nan")),
                             ("sigma_div", 0.0), ("proj", 4), ("proj", 0)):
            assert set_variants([good[0], bad(**{field: value})]) == MPPI_EINVAL, (field, value)
            msg = lib.mppi_last_error()
            assert b"row 1" in msg and field.encode() in msg, msg
        assert set_variants(good, n=1025) == MPPI_EINVAL
        assert set_variants(good, n=-1) == MPPI_EINVAL
        assert lib.mppi_batch_set_variants(batch.h, 2, None) == MPPI_EINVAL
        assert lib.mppi_batch_variant_default(batch.h, 5, C.byref(_policy()), C.byref(good[0])) == MPPI_EINVAL
        # the table and the indices are as before the refused calls
        batch.run(V.CAP, "3d", _policy())
        V.same(V.collect(batch, 0), V.ref_a_named("temperature3"), "episode 0 after the refused calls")
        V.same(V.collect(batch, 1), V.ref_a_named("proj2d"), "episode 1 after the refused calls")
        # clearing the table needs the indices released first
        for e in range(2):
            assert lib.mppi_batch_set_episode_variant(batch.h, e, -1) == 0
        assert set_variants([]) == 0
        assert lib.mppi_batch_set_episode_variant(batch.h, 0, 0) == MPPI_EINVAL
        batch.close()
    finally:
        eng.close()
