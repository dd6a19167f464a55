"""GPU: on-device scoring of the batched episodes' executed paths (mppi_batch_score).

Batch.score() must give, for every episode, the bits of mppi_score_paths called on the episode's log
(traj = columns 0-2, lin_vel = column 6, no wheel arrays) with the same origin; three episodes are
also checked against oracle.mppi_ref.critics directly.  K = 256, H = 20, the C3 scene.
"""
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V

pytestmark = pytest.mark.gpu

F32 = np.float32
HORIZON = 0.045 * 2.0 * V.H       # make_params' default: dt * v_max_linear * H
E_BIG, SEEDS_EACH = 70, 14        # two tiles of 64 paths, the second partial


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _policy():
    from mppi_amd import _lib
    return _lib.make_policy(**B.RUN)


def _set(batch, episodes):
    for e, (start, goal, seed) in enumerate(episodes):
        batch.set_episode(e, V.mppi_state(B.start_state(start, goal)), seed)


def _origins(episodes):
    return [V.origin_state(s[0], s[1], g[0], g[1]) for s, g, _ in episodes]


def _big_episodes():
    return [(start, goal, 100 * i + j) for i, (start, goal, _, _) in enumerate(B.MAIN) for j in range(SEEDS_EACH)]


@functools.lru_cache(maxsize=None)
def _big():
    """The E = 70 batch: the MAIN starts and goals with 14 seeds each, cap 40; its logs and scores."""
    _gpu()
    from mppi_amd import _lib
    eps = _big_episodes()
    assert len(eps) == E_BIG
    eng = V.make_engine()
    try:
        batch = _lib.Batch(eng, E_BIG)
        _set(batch, eps)
        batch.run(40, "3d", _policy())
        logs = [batch.log(e) for e in range(E_BIG)]
        got = batch.score()
        ms = eng.score_ms()
        want = [V.score_one(eng, logs[e], o) for e, o in enumerate(_origins(eps))]
        batch.close()
    finally:
        eng.close()
    return eps, logs, got, want, ms


def test_score_matches_score_paths():
    eps, logs, got, want, ms = _big()
    lengths = [len(r) for r in logs]
    print("path lengths:", sorted(set(lengths)), "score kernel ms:", ms)
    assert ms > 0.0
    assert 0 in lengths and 40 in lengths and len(set(lengths)) >= 3
    dist = [np.hypot(g[0] - s[0], g[1] - s[1]) for s, g, _ in eps]
    assert any(d > HORIZON and d >= 2.0 for d in dist)     # far path-follow branch, speed critic on
    assert any(d <= HORIZON and d < 2.0 for d in dist)     # near branch, speed critic off
    assert list(got["rows"]) == lengths
    for e in range(E_BIG):
        w = want[e]
        assert F32(got["cost"][e]).view(np.uint32) == F32(w["cost"]).view(np.uint32), (e, got["cost"][e], w["cost"])
        assert np.array_equal(got["terms"][e].view(np.uint32), np.asarray(w["terms"], F32).view(np.uint32)), \
            (e, got["terms"][e], w["terms"])
        assert got["collisions"][e] == w["collisions"], e
        if lengths[e] == 0:
            assert got["cost"][e] == 0 and not got["terms"][e].any() and got["collisions"][e] == 0
    far = [e for e in range(E_BIG) if lengths[e] == 40]
    assert all(got["terms"][e, 2] > 0 for e in far)        # the speed critic ran


def test_lengths_around_the_chunk():
    """Path lengths around the kernel's chunk of 12 waypoints: one far-goal batch of 3 episodes run with
    caps 1, 2, 3, 4, 11, 12, 13 and 25, the episodes set again between runs."""
    _gpu()
    from mppi_amd import _lib
    eps = [(B.START, V.FAR, 1), (B.START, V.FAR, 2), ((10.0, 12.0), V.FAR, 3)]
    eng = V.make_engine()
    try:
        batch = _lib.Batch(eng, len(eps))
        for cap in (1, 2, 3, 4, 11, 12, 13, 25):
            _set(batch, eps)
            batch.run(cap, "3d", _policy())
            logs = [batch.log(e) for e in range(len(eps))]
            assert all(len(r) == cap for r in logs)
            V.check_scores(batch.score(), eng, logs, _origins(eps), f"cap {cap}")
        _set(batch, eps)    # set again and not run: no rows
        got = batch.score()
        assert not got["rows"].any() and not got["cost"].any() and not got["terms"].any()
        batch.close()
    finally:
        eng.close()


def test_yardstick_and_origins():
    """A yardstick with other weights, threshold 0.5 and penalty 1000 against a second engine created
    with those params; explicit per-episode origins, one of them within 2 m of its goal between far
    neighbours, so the lanes of one wave take different branches."""
    _gpu()
    from mppi_amd import _lib
    from mppi_amd.batch import variant_dict
    eps = [(B.START, V.FAR, s) for s in (1, 2, 3)] + [(V.COLLISION_START, V.FAR, 4), (V.COLLISION_START, V.FAR, 5)]
    other = dict(w_path=3.0, w_slope=7.0, w_speed=11.0, w_obstacle=0.25, collision_threshold=0.5,
                 collision_penalty=1000.0)
    eng = V.make_engine()
    eng2 = V.make_engine(**other)
    try:
        batch = _lib.Batch(eng, len(eps))
        _set(batch, eps)
        batch.run(13, "3d", _policy())
        logs = [batch.log(e) for e in range(len(eps))]
        origins = _origins(eps)
        got = batch.score(yardstick=variant_dict("3d", **other))
        V.check_scores(got, eng2, logs, origins, "yardstick")
        plain = batch.score()
        assert not np.array_equal(plain["cost"], got["cost"])
        assert np.array_equal(plain["terms"][:, :3], got["terms"][:, :3])
        # explicit origins: episode 1 measured from 1 m before its goal (near branch, speed critic off)
        explicit = list(origins)
        explicit[0] = V.origin_state(-50.0, 0.0, 60.0, 12.0)
        explicit[1] = V.origin_state(V.FAR[0] - 1.0, V.FAR[1], V.FAR[0], V.FAR[1])
        explicit[3] = V.origin_state(-38.0, 39.0, -36.1, 39.0)   # 1.9 m: beyond the horizon (1.8 m), speed critic off
        got = batch.score(origins=explicit)
        V.check_scores(got, eng, logs, explicit, "origins")
        assert got["terms"][1, 2] == 0 and got["terms"][3, 2] == 0
        assert got["terms"][0, 2] > 0 and got["terms"][2, 2] > 0 and got["terms"][4, 2] > 0
        got = batch.score(yardstick=_lib.make_variant(**variant_dict("2d", **other)), origins=explicit)
        V.check_scores(got, eng2, logs, explicit, "yardstick and origins")
        batch.close()
    finally:
        eng2.close()
        eng.close()


def test_score_matches_oracle():
    """Terms and collisions of three episodes (a short path, one ended by the goal test, one at the cap)
    equal oracle.mppi_ref.critics on the logged path in body-slope mode."""
    eps, logs, got, _, _ = _big()
    lengths = np.array([len(r) for r in logs])
    short = int(np.argmin(np.where(lengths > 0, lengths, 1000)))
    mid = int(np.argmax(np.where(lengths < 40, lengths, -1)))
    cap = int(np.argmax(lengths == 40))
    assert 0 < lengths[short] <= lengths[mid] < 40 == lengths[cap]
    for e in (short, mid, cap):
        start, goal, _ = eps[e]
        terms, col = V.oracle_terms(logs[e], start, goal, HORIZON)
        assert np.array_equal(got["terms"][e].view(np.uint32), terms.view(np.uint32)), (e, got["terms"][e], terms)
        assert got["collisions"][e] == col, e


def test_score_changes_no_state():
    """A batch run continued after score() gives the bits of one not scored in between."""
    _gpu()
    from mppi_amd import _lib
    eps = [(start, goal, seed) for start, goal, seed, _ in B.MAIN]
    out = {}
    for scored in (False, True):
        eng = V.make_engine()
        try:
            batch = _lib.Batch(eng, len(eps))
            _set(batch, eps)
            batch.run(8, "3d", _policy())
            first = [batch.log(e) for e in range(len(eps))]
            if scored:
                batch.score()
                assert all(np.array_equal(batch.log(e), first[e]) for e in range(len(eps)))
            batch.run(8, "3d", _policy())
            out[scored] = [V.collect(batch, e) for e in range(len(eps))]
            batch.close()
        finally:
            eng.close()
    for e in range(len(eps)):
        V.same(out[True][e], out[False][e], f"episode {e}")
        assert out[True][e]["total"] == out[False][e]["total"]
