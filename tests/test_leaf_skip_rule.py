"""CPU: the rule by which the rollout's leaf reduction skips lines of zero weights.

A leaf's 256 trajectories are eight lines of 32.  A line whose 32 weights are all 0.0f is neither
loaded nor multiplied: its sum (a tree of products 0 * u, +0 or -0) is taken as +0.0.  Every node of
the tree is then its true value or a zero whose true value is a zero too, so a row that does not
compare equal to 0.0 has its true bits; a row that does is summed again with all eight lines.

This file restates that rule in numpy and compares it bit for bit with oracle.mppi_ref.leaf_records,
which multiplies everything: on a real-scene step at four temperatures, and on a set built so that the
rule WITHOUT the recompute differs (so the recompute is shown to be needed, and exercised).
"""
import functools

import numpy as np

import helpers as hp
from oracle import dmath
from oracle import mppi_ref as R

F32 = np.float32
LINE = 32


def _weights(cost, temperature):
    """The leaf weights exactly as oracle.mppi_ref.leaf_records forms them: [nleaf, 256] float32."""
    nleaf = (cost.size + R.LEAF - 1) // R.LEAF
    c = np.concatenate([cost.astype(F32), np.full(nleaf * R.LEAF - cost.size, np.inf, F32)]).reshape(nleaf, R.LEAF)
    m = c.min(axis=1)
    finite = np.isfinite(c)
    safe_m = np.where(np.isfinite(m), m, F32(0.0)).astype(F32)
    diff = np.where(finite, c - safe_m[:, None], F32(0.0)).astype(F32)
    w = np.where(finite, dmath.dm_expf(-(diff / F32(temperature))), F32(0.0)).astype(F32)
    return m, w


def _tree(x):
    """Pairwise tree over axis 1 in index order."""
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def leaf_records_skip(cost, u1, u2, temperature, recompute=True):
    """leaf_records under the skip rule: +0.0 for a dead line; rows equal to zero summed densely."""
    Kn, H = u1.shape
    m, w = _weights(cost, temperature)
    nleaf = w.shape[0]
    pad = nleaf * R.LEAF - Kn
    rows = [np.ones((nleaf, R.LEAF, 1))]                                   # S: the weights alone
    for u in (u1, u2):
        rows.append(np.concatenate([u, np.zeros((pad, H), F32)]).reshape(nleaf, R.LEAF, H).astype(np.float64))
    prod = w.astype(np.float64)[:, :, None] * np.concatenate(rows, axis=2)  # [nleaf, 256, 1 + 2H]
    nrow = prod.shape[2]
    lines = prod.reshape(nleaf, R.LEAF // LINE, LINE, nrow)
    line_sum = np.stack([_tree(lines[:, k]) for k in range(R.LEAF // LINE)], axis=1)   # [nleaf, 8, nrow]
    live = (w.reshape(nleaf, R.LEAF // LINE, LINE) != 0).any(axis=2)                    # [nleaf, 8]
    skipped = np.where(live[:, :, None], line_sum, np.float64(0.0))
    out = _tree(skipped)
    if recompute:
        out = np.where(out == 0.0, _tree(line_sum), out)
    rec = np.empty((nleaf, 2 * H + 2), np.float64)
    rec[:, 0] = m.astype(np.float64)
    rec[:, 1:] = out
    return rec, live


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


@functools.lru_cache(maxsize=1)
def _scene_step():
    """One step on the C3 scene (K = 1280: five leaves, H = 100)."""
    K, H = 1280, 100
    Z, hw, cm = hp.c3_scene()
    p = R.Params(K=K, H=H, seed=42)
    r = R.rollout_costs(p, hp.oracle_scene(Z, hw, cm), hp.oracle_state(), np.zeros(H, F32), np.zeros(H, F32), 0,
                        np.arange(K, dtype=np.int64))
    return r["cost"], r["u1"], r["u2"]


def test_skip_rule_on_a_scene_step():
    cost, u1, u2 = _scene_step()
    seen = {}
    for T in (0.3, 30.0, 3000.0, 1e5):
        want = R.leaf_records(cost, u1, u2, T)
        got, live = leaf_records_skip(cost, u1, u2, T)
        assert np.array_equal(_bits(got), _bits(want)), (T, hp.mismatch_report("record", got, want))
        seen[T] = live.sum(axis=1)
    assert seen[0.3].max() <= 2, seen        # the controller's temperature: nearly every line is dead
    assert seen[1e5].min() == 8, seen        # every line live: nothing is skipped


def _adversarial(seed):
    rng = np.random.RandomState(seed)
    nleaf, H = 12, 8
    K = nleaf * R.LEAF - 100                  # a ragged last leaf
    cost = (rng.uniform(0.0, 40000.0, K)).astype(F32)   # (mostly one live trajectory per leaf at T = 0.3)
    cost[rng.rand(K) < 0.2] = np.inf
    cost[2 * R.LEAF:3 * R.LEAF] = np.inf      # all-infinite leaves (live mask 0)
    cost[7 * R.LEAF:8 * R.LEAF] = np.inf
    vals = np.array([-1.0, -0.0, 0.0, 0.5, -0.25], F32)
    u1 = vals[rng.randint(0, 5, (K, H))]
    u2 = vals[rng.randint(0, 5, (K, H))]
    neg = np.array([-1.0, -0.0, -0.25], F32)  # columns of negative signs only: a row of true value -0.0
    u1[:, :3] = neg[rng.randint(0, 3, (K, 3))]
    u2[:, 5:] = neg[rng.randint(0, 3, (K, H - 5))]
    for leaf in range(nleaf):                 # the minimum-cost trajectory's rows: -0.0
        c = cost[leaf * R.LEAF:(leaf + 1) * R.LEAF]
        if np.isfinite(c).any():
            k = leaf * R.LEAF + int(np.argmin(c))
            u1[k] = F32(-0.0)
            u2[k] = F32(-0.0)
    return cost, u1, u2


def test_skip_rule_needs_the_zero_row_recompute():
    differ = 0
    for seed in range(4):
        cost, u1, u2 = _adversarial(seed)
        want = R.leaf_records(cost, u1, u2, 0.3)
        got, live = leaf_records_skip(cost, u1, u2, 0.3)
        assert np.array_equal(_bits(got), _bits(want)), (seed, hp.mismatch_report("record", got, want))
        assert (live.sum(axis=1) == 0).sum() >= 2 and live.any()
        bare, _ = leaf_records_skip(cost, u1, u2, 0.3, recompute=False)
        bad = _bits(bare) != _bits(want)
        assert (bare[bad] == 0.0).all() and (want[bad] == 0.0).all()   # only the sign of a zero can differ
        differ += int(bad.sum())
    assert differ > 0, "the set does not exercise the recompute"
