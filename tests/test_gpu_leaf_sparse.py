"""GPU: the leaf reduction's live mask against the oracle, bit for bit.

leaf_records loads and multiplies only the 32-trajectory lines that hold a non-zero softmax weight,
takes the dense layout when every line is live, and sums a row that comes out equal to 0.0 again with
every line (the sign of the zero).  The cases: sparse, dense and mixed leaves on both rollout kernels,
one leaf / a ragged last leaf / several leaves, rows served by the LDS control cache and rows re-read
from the normals (H = 100) or all cached (H = 20); rows of true value -0.0 and +0.0 through injected
controls; the resident server against separate launches.  Each case first asserts on the oracle's
weights that its leaves are what it claims.
"""
import functools

import numpy as np
import pytest

import helpers as hp
from oracle import dmath
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 42
T_SPARSE = 0.3                      # the controller's temperature
T_DENSE = 3000.0                    # every line that holds a trajectory is live (asserted below)
T_MIXED = {100: 1000.0, 20: 10.0}   # some leaf with 3..6 live lines (asserted below)
FLOATS = ("u1_opt", "u2_opt", "lin_vel", "ang_vel", "traj_sim", "heading_sim", "left_wheel_sim", "right_wheel_sim")
REF = dict(u1_opt="u1_opt", u2_opt="u2_opt", lin_vel="v_opt", ang_vel="w_opt", traj_sim="traj_sim",
           heading_sim="hv_sim", left_wheel_sim="lw_sim", right_wheel_sim="rw_sim")


@pytest.fixture(params=["roles", "pair"])
def rollout_kernel(request, monkeypatch):
    """Both rollout kernels, forced by MPPI_ROLES, which a context reads when it is created."""
    monkeypatch.setenv("MPPI_ROLES", "1" if request.param == "roles" else "0")
    return request.param


def _u32(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _live_lines(cost, T):
    """Live 32-trajectory lines of every leaf, from the oracle's weights: [nleaf, 8] bool."""
    nleaf = (cost.size + R.LEAF - 1) // R.LEAF
    c = np.concatenate([cost.astype(F32), np.full(nleaf * R.LEAF - cost.size, np.inf, F32)]).reshape(nleaf, R.LEAF)
    fin = np.isfinite(c)
    m = np.where(fin.any(axis=1), c.min(axis=1), F32(0.0)).astype(F32)
    diff = np.where(fin, c - m[:, None], F32(0.0)).astype(F32)
    w = np.where(fin, dmath.dm_expf(-(diff / F32(T))), F32(0.0)).astype(F32)
    return (w.reshape(nleaf, 8, 32) != 0).any(axis=2)


@functools.lru_cache(maxsize=None)
def _oracle(K, H, T):
    Z, hw, cm = hp.c3_scene()
    p = R.Params(K=K, H=H, seed=SEED, temperature=T)
    ref = R.mppi_step(p, hp.oracle_scene(Z, hw, cm), hp.oracle_state(), np.zeros(H, F32), np.zeros(H, F32), 0)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _assert_bitwise(out, costs, ref, tag):
    assert np.array_equal(_u32(costs), _u32(ref["cost"])), hp.mismatch_report(f"{tag} cost", costs, ref["cost"])
    for a in FLOATS:
        assert np.array_equal(_u32(out[a]), _u32(ref[REF[a]])), hp.mismatch_report(f"{tag} {a}", out[a], ref[REF[a]])


def _check_ucache(eng, H):
    n = eng.launch_info()["ucache_steps"]
    if H == 100:
        assert 0 < n < H, n      # rows beyond the control cache are re-read from the normals
    else:
        assert n == H, n         # every row comes from the control cache


def _step_case(K, H, T, kind):
    ref = _oracle(K, H, T)
    live = _live_lines(ref["cost"], T)
    per_leaf = live.sum(axis=1)
    if kind == "sparse":
        assert per_leaf.max() <= 2, per_leaf
    elif kind == "dense":   # (a ragged last leaf has lines without a trajectory: those can never be live)
        holds = (np.arange(live.size).reshape(live.shape) * 32) < K
        assert np.array_equal(live, holds), per_leaf
        assert per_leaf[0] == 8
    else:
        assert ((per_leaf >= 3) & (per_leaf <= 6)).any(), per_leaf
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state()
    eng = hp.engine_for(K, H, Z, hw, cm, st, seed=SEED, temperature=T)
    try:
        out = eng.step("3d", 0)
        _check_ucache(eng, H)
        _assert_bitwise(out, eng.costs(), ref, f"{kind} K={K} H={H}")
    finally:
        eng.close()
    if K != 256:
        return
    import torch   # the leaf record itself (a fresh engine: the step above handed its nominal sequence on)
    eng = hp.engine_for(K, H, Z, hw, cm, st, seed=SEED, temperature=T)
    try:
        if True:  # (kept as a block)
            rec = torch.empty(eng.record_len(), dtype=torch.float64, device="cuda:0")
            eng.step_partial(rec.data_ptr(), "3d", 0)
            torch.cuda.synchronize()
            p = R.Params(K=K, H=H, seed=SEED, temperature=T)
            want, _ = R.shard_record(p, hp.oracle_scene(Z, hw, cm), st, np.zeros(H, F32), np.zeros(H, F32), 0, 0, K)
            got = rec.cpu().numpy()
            assert np.array_equal(got.view(np.int64), np.ascontiguousarray(want).view(np.int64)), \
                hp.mismatch_report("record", got, want)
    finally:
        eng.close()


@pytest.mark.parametrize("H", [100, 20])
@pytest.mark.parametrize("K", [256, 300, 1280])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_sparse_and_dense_leaves(rollout_kernel, kind, K, H):
    _step_case(K, H, T_SPARSE if kind == "sparse" else T_DENSE, kind)


@pytest.mark.parametrize("H", [100, 20])
@pytest.mark.parametrize("K", [256, 300, 1280])
def test_mixed_leaf(rollout_kernel, K, H):
    _step_case(K, H, T_MIXED[H], "mixed")


@pytest.mark.parametrize("K,H", [(256, 100), (1280, 100), (1280, 20)])
@pytest.mark.parametrize("elsewhere", ["negative", "forward"])
def test_zero_rows_keep_their_sign(rollout_kernel, elsewhere, K, H):
    """Rows whose true sum is -0.0 (u1) and +0.0 (u2): the skipped lines' +0.0 would turn -0.0 into
    +0.0; such rows are summed again with every line.  "negative": negative controls in every other
    row (the rover, commanded backwards, stands still: many trajectories tie at the minimum cost and
    every line is live).  "forward": the rover drives, the costs spread and the leaves are sparse, so
    the zero rows take the recompute.  (Whole leaves only: the oracle pads a ragged leaf with +0.0
    controls, the engine's rows hold what was injected, so there the sign of a zero row is not defined
    alike on both sides, with or without the live mask.)"""
    rng = np.random.RandomState(1)
    if elsewhere == "negative":
        u1 = rng.uniform(-1.0, -0.1, (K, H)).astype(F32)
        u2 = rng.uniform(-1.0, -0.1, (K, H)).astype(F32)
    else:
        u1 = rng.uniform(0.1, 1.0, (K, H)).astype(F32)
        u2 = rng.uniform(-1.0, 1.0, (K, H)).astype(F32)
    t_neg, t_pos = [0, 7, H // 2, H - 1], [1, 8, H // 2 + 1, H - 2]
    u1[:, t_neg] = F32(-0.0)
    u2[:, t_pos] = F32(0.0)
    Z, hw, cm = hp.c3_scene()
    st = hp.oracle_state()
    p = R.Params(K=K, H=H)
    ref = R.mppi_step(p, hp.oracle_scene(Z, hw, cm), st, np.zeros(H, F32), np.zeros(H, F32), 0, injected=(u1, u2))
    if elsewhere == "forward":
        per_leaf = _live_lines(ref["cost"], p.temperature).sum(axis=1)
        assert per_leaf.max() <= 2, per_leaf
    V1, V2 = ref["root"][2:2 + H], ref["root"][2 + H:]
    assert (V1[t_neg] == 0.0).all() and np.signbit(V1[t_neg]).all(), V1[t_neg]
    assert (V2[t_pos] == 0.0).all() and not np.signbit(V2[t_pos]).any(), V2[t_pos]
    others = np.setdiff1d(np.arange(H), t_neg)
    assert (V1[others] != 0.0).all()
    eng = hp.engine_for(K, H, Z, hw, cm, st)
    try:
        out = eng.step_injected(u1, u2)
        _assert_bitwise(out, eng.costs(), ref, f"zero rows {elsewhere} K={K} H={H}")
    finally:
        eng.close()


def test_server_equals_separate_launches():
    """Three chained steps at K = 1280, H = 100 on the resident server against one launch per kernel."""
    K, H = 1280, 100
    Z, hw, cm = hp.c3_scene()

    def run(resident):
        eng = hp.engine_for(K, H, Z, hw, cm, hp.oracle_state(), seed=SEED)
        eng.set_option("resident", resident)
        outs = []
        try:
            for i in range(3):
                eng.step("3d", i, copy=False)
                o = eng.outputs()
                outs.append({k: o[k].copy() for k in FLOATS})
            return outs, eng.costs(), eng.launch_info()
        finally:
            eng.close()

    got, gc, gi = run(2)
    want, wc, wi = run(0)
    assert gi["resident"] == 1 and gi["server_steps"] == 3, gi
    assert wi["resident"] == 0, wi
    assert np.array_equal(_u32(gc), _u32(wc))
    for i, (a, b) in enumerate(zip(got, want)):
        for k in FLOATS:
            assert np.array_equal(_u32(a[k]), _u32(b[k])), hp.mismatch_report(f"step {i} {k}", a[k], b[k])
