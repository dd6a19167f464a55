"""CPU: the oracle's softmax reduction on costs that are not finite.

The rule, as DESIGN.md states it, restated here as scalar float64 loops that share no code with
oracle.mppi_ref.leaf_records / combine / tree_reduce:

  * a cost that is NaN (either sign), +inf or -inf is dead: weight 0, and it enters no minimum;
  * a leaf's m is the smallest of its finite costs, +inf when it has none; then S = 0 and V = 0;
  * a record whose m is not finite is empty: at a node it passes its sibling through (an empty left
    child gives the right child as it stands, even when that one is empty too);
  * no finite cost at all: u_opt is +0.0 everywhere.

Cases: 1, 2 and 5 leaves (and a ragged K = 300); in every leaf one dead lane; one dead 32-line; one
dead half; a whole leaf dead; all lanes but one dead; everything dead; each with +NaN, -NaN, +inf
and -inf, at the sparse (T = 0.3) and the dense (T = 3000) temperature.  m, S and V equal bitwise.
"""
import numpy as np
import pytest

from nonfinite_refs import NEG_NAN, PATTERNS, POS_NAN, dead_set
from oracle import dmath
from oracle import mppi_ref as R

F32 = np.float32
H = 5
KINDS = {"+nan": POS_NAN, "-nan": NEG_NAN, "+inf": F32(np.inf), "-inf": F32(-np.inf)}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


# ------------------------------------------------------------------ the rule, scalar
def _tree_sum(xs):
    """((x0 + x1) + (x2 + x3)) + ... in float64, index order, length a power of two."""
    if len(xs) == 1:
        return xs[0]
    h = len(xs) // 2
    return _tree_sum(xs[:h]) + _tree_sum(xs[h:])


def _expf(x):
    return float(dmath.dm_expf(np.array([x], F32))[0])


def scalar_leaf(cost, u1, u2, T):
    """One leaf of up to 256 trajectories -> [m, S, V1[0:H], V2[0:H]] as floats."""
    T = F32(T)
    n = len(cost)
    m = F32(np.inf)
    for c in cost:
        if np.isfinite(c) and c < m:
            m = F32(c)
    w = [0.0] * R.LEAF
    live = [k for k in range(n) if np.isfinite(cost[k])]
    if live:   # (dm_expf, the shared float32 exponential, once for the leaf's live lanes)
        e = dmath.dm_expf(np.array([-((F32(cost[k]) - m) / T) for k in live], F32))
        for k, x in zip(live, e):
            w[k] = float(x)
    rec = [float(m), _tree_sum(w)]
    for u in (u1, u2):
        for t in range(u.shape[1]):
            rec.append(_tree_sum([w[k] * float(u[k, t]) if k < n else w[k] * 0.0 for k in range(R.LEAF)]))
    return rec


def scalar_combine(a, b, T):
    T = F32(T)
    ma, mb = F32(a[0]), F32(b[0])
    if not np.isfinite(ma):
        return list(b)
    if not np.isfinite(mb):
        return list(a)
    m = ma if ma <= mb else mb
    ea = _expf(-((ma - m) / T))
    eb = _expf(-((mb - m) / T))
    return [float(m)] + [ea * x + eb * y for x, y in zip(a[1:], b[1:])]


def scalar_tree(recs, T):
    recs = [list(r) for r in recs]
    width = len(recs[0])
    n = 1
    while n < len(recs):
        n *= 2
    recs += [[float("inf")] + [0.0] * (width - 1) for _ in range(n - len(recs))]
    while len(recs) > 1:
        recs = [scalar_combine(recs[i], recs[i + 1], T) for i in range(0, len(recs), 2)]
    return recs[0]


def scalar_records(cost, u1, u2, T):
    out = []
    for b in range(0, len(cost), R.LEAF):
        out.append(scalar_leaf(cost[b:b + R.LEAF], u1[b:b + R.LEAF], u2[b:b + R.LEAF], T))
    return out


# ------------------------------------------------------------------ the cases
def _inputs(K, seed=0):
    rng = np.random.RandomState(seed)
    cost = rng.uniform(10.0, 5000.0, K).astype(F32)
    u1 = rng.uniform(-1.0, 1.0, (K, H)).astype(F32)
    u2 = rng.uniform(-1.0, 1.0, (K, H)).astype(F32)
    return cost, u1, u2


@pytest.mark.parametrize("T", [0.3, 3000.0])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", [256, 512, 1280, 300])
def test_leaf_records_and_tree_follow_the_rule(K, pattern, kind, T):
    cost, u1, u2 = _inputs(K)
    dead = dead_set(pattern, K)
    assert dead.any()
    cost[dead] = KINDS[kind]
    got = R.leaf_records(cost, u1, u2, T)
    want = np.array(scalar_records(cost, u1, u2, T), np.float64)
    assert np.array_equal(_bits(got), _bits(want)), (got[:, :2], want[:, :2])
    # what the text says of the record of a leaf with no finite cost
    nleaf = got.shape[0]
    c = np.concatenate([cost, np.full(nleaf * R.LEAF - K, np.inf, F32)]).reshape(nleaf, R.LEAF)
    for q in range(nleaf):
        if not np.isfinite(c[q]).any():
            assert np.array_equal(_bits(got[q]), _bits(R.empty_record(H)))
        else:
            assert got[q, 0] == c[q][np.isfinite(c[q])].min() and got[q, 1] >= 1.0
    root = R.tree_reduce(got, T)
    assert np.array_equal(_bits(root), _bits(np.array(scalar_tree(want, T))))
    a, b = R.u_opt_from_root(root, H)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    if dead.all():   # ("all", and the one leaf of K = 256 under "leaf")
        z = np.zeros(H, F32).view(np.uint32)
        assert np.array_equal(a.view(np.uint32), z) and np.array_equal(b.view(np.uint32), z)   # +0.0, not -0.0
    else:
        assert root[1] > 0.0 and np.isfinite(root[0])
        assert np.all(np.abs(a) <= 1.0) and np.all(np.abs(b) <= 1.0)


def test_mixed_kinds_in_one_leaf():
    """All four kinds in one leaf beside finite costs, and a smaller finite cost after a -inf."""
    cost, u1, u2 = _inputs(512, seed=3)
    cost[[3, 40, 77, 255, 256, 300]] = [NEG_NAN, F32(-np.inf), POS_NAN, F32(np.inf), F32(-np.inf), F32(1.0)]
    for T in (0.3, 3000.0):
        got = R.leaf_records(cost, u1, u2, T)
        want = np.array(scalar_records(cost, u1, u2, T))
        assert np.array_equal(_bits(got), _bits(want))
        assert got[1, 0] == 1.0 and np.isfinite(got[0, 0])


def test_finite_costs_are_untouched():
    """Finite costs: the record is what the unmasked minimum gives (the rule changes no finite result)."""
    cost, u1, u2 = _inputs(1280, seed=5)
    got = R.leaf_records(cost, u1, u2, 0.3)
    assert np.array_equal(got[:, 0], cost.reshape(5, 256).min(axis=1).astype(np.float64))
    assert np.array_equal(_bits(got), _bits(np.array(scalar_records(cost, u1, u2, 0.3))))


def _crafted(m, seed, S=None):
    rng = np.random.RandomState(seed)
    r = rng.uniform(-2.0, 2.0, 2 * H + 2)
    r[0] = m
    r[1] = rng.uniform(0.5, 3.0) if S is None else S
    return r


M_KINDS = {"finite": 12.5, "finite2": 14.0, "+inf": np.inf, "-inf": -np.inf, "+nan": float(POS_NAN),
           "-nan": float(NEG_NAN)}


@pytest.mark.parametrize("T", [0.3, 3000.0])
@pytest.mark.parametrize("kb", list(M_KINDS))
@pytest.mark.parametrize("ka", list(M_KINDS))
def test_combine_both_orders(ka, kb, T):
    """Every pair of m kinds, which is both argument orders of each; empty sides carry garbage S, V."""
    a, b = _crafted(M_KINDS[ka], 1), _crafted(M_KINDS[kb], 2)
    got = R.combine(a, b, T)
    want = np.array(scalar_combine(a, b, T))
    assert np.array_equal(_bits(got), _bits(want)), (ka, kb, got, want)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_tree_with_dead_members(n):
    """A dead member (m NaN / +inf / -inf, or finite with S = 0) at the first, middle and last place."""
    T = 0.3
    for kind in ("+nan", "-nan", "+inf", "-inf", "S=0"):
        for pos in sorted({0, n // 2, n - 1}):
            recs = [_crafted(20.0 + 0.1 * i, 10 + i) for i in range(n)]
            if kind == "S=0":
                recs[pos] = np.concatenate([[19.0, 0.0], np.zeros(2 * H)])
            else:
                recs[pos] = _crafted(M_KINDS[kind], 99)
            got = R.tree_reduce(np.stack(recs), T)
            want = np.array(scalar_tree(recs, T))
            assert np.array_equal(_bits(got), _bits(want)), (n, kind, pos)
    empties = np.stack([R.empty_record(H)] * n)
    root = R.tree_reduce(empties, T)
    assert np.array_equal(_bits(root), _bits(R.empty_record(H)))
    a, b = R.u_opt_from_root(root, H)
    assert not a.any() and not b.any() and not np.signbit(a).any() and not np.signbit(b).any()


def test_clamp_returns_the_lower_bound_for_nan():
    """D13: clamp is fmin(fmax(x, lo), hi), so clamp(NaN) = lo and ±inf go to the matching bound."""
    x = np.array([POS_NAN, NEG_NAN, np.inf, -np.inf, 0.25], F32)
    got = R.clampf(x, F32(-1.0), F32(2.0))
    assert np.array_equal(got.view(np.uint32), np.array([-1.0, -1.0, 2.0, -1.0, 0.25], F32).view(np.uint32))


def test_cell_of_a_nonfinite_coordinate():
    """D13: NaN clamps to the lower bound of the float clamp, ±inf to the matching one (IEEE division)."""
    sc = R.Scene(np.zeros((7, 9), F32), 4.5, np.zeros((4, 4), F32))
    x = np.array([POS_NAN, NEG_NAN, np.inf, -np.inf, 3e38, -3e38], F32)
    i, j = R.dem_cell(sc, x, x)
    assert i.tolist() == [-1, -1, 9, -1, 9, -1]
    assert j.tolist() == [7, 7, -1, 7, -1, 7]


def test_a_nan_pose_is_not_reached():
    """D13: the goal test is 'inside the tolerance on both axes'; a NaN coordinate is never inside, in
    mppi_amd.batch.is_active and in the references' loop condition alike.  Finite cases keep their answer."""
    import batch_refs as B
    from mppi_amd import batch
    nan = float("nan")
    for x, y, active in ((nan, nan, True), (nan, 0.0, True), (0.0, nan, True), (0.2, -0.3, False), (0.5, -0.5, False),
                         (0.6, 0.0, True), (0.0, -0.6, True), (float("inf"), 0.0, True)):
        assert batch.is_active(batch.state_dict(x, y, goal_x=0.0, goal_y=0.0)) == active, (x, y)
        assert B.active(B.start_state((x, y), (0.0, 0.0)), B.RUN) == active, (x, y)
