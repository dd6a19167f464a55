"""GPU: the 64-bit sampling key: seeds, steps and trajectory indices off the low word.

Every sampling normal is one Philox block with counter (n lo, n hi, k lo, k hi) and key (seed lo,
seed hi), n = step * ceil(H/2) + t/2 modulo 2^64 and k = k_offset + trajectory.  The words reach the
device through seven generators: the engine's plain, plan and serial noise kernels, the resident
server's noise phase (with and without a plan, fed from the command's noise_n_base_lo / _hi) and the
batch's two noise kernels.  The engine's three run with each word wide: beyond 2^32, with the 2^32
line inside one wave and inside one step, at 2^63 and over the wrap at 2^64.  The server's phase
runs with a wide seed over step sequences that carry, leave the signed range, wrap and jump.  The
batch's plain kernel and the three generators inside its plan kernel run with wide seeds (a
batch's trajectory offset is its context's and its step index counts from 0).

Every comparison is bitwise against the oracle: tests/sampling_refs.py's controls from
oracle.dmath.noise at the case's seed, step and global indices, the oracle's step on them, and the
engine's dumped u1 / u2 against the sampled controls themselves.  Every case first asserts on the
oracle's own arrays that the wide word matters (the normals differ from those with the high word
cleared, in the rows and columns where they must), that at least 99 % of the sampled controls lie
strictly inside their bounds (a clamped sample hides its normal) and that costs and outputs are finite.

Shapes: K = 300, H = 5 (two ragged leaves, odd H, three blocks per step); K = 768 and K = 4096 on the
resident server (at K = 4096, 16 records, the server's own noise phase generates step + 2, which the
test asserts from launch_info by server_step's rule; at K = 768 the noise kernel does); a batch of
E = 3, K = 256, once without any sampling row (the plain batch kernel) and once with rows (the plan
kernel); a group of two members of 256 around k = 2^32.  C3 scene throughout.
"""
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V
import helpers as hp
import sampling_refs as SR
import wide_key_cases as WK
from mppi_amd import sampling as S
from oracle import dmath
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
M32, M64 = 0xFFFFFFFF, WK.M64
H, GOLDEN, S0, PLANS, CASES = WK.H, WK.GOLDEN, WK.S0, WK.PLANS, WK.CASES
NB = (H + 1) // 2
# The closed loops (sections b and c) run with control bounds of +-4 instead of +-1: fed back, the
# nominal sequence reaches 1 within three steps on this scene (the controller asks for full speed), and at the default bounds
# 12 to 26 % of the samples of the later steps would be clamped, on the oracle as on any engine.  With
# +-4 every step of every sequence keeps the 99 % precondition (asserted step by step in _expected);
# the velocity limits are the default ones, so the rollouts are as tame as ever.
LOOP_BOUNDS = dict(min_u1=-4.0, max_u1=4.0, min_u2=-4.0, max_u2=4.0)


# ------------------------------------------------------------------ the oracle's side (no GPU)
@functools.lru_cache(maxsize=None)
def _scene():
    return hp.oracle_scene(*hp.c3_scene())


def _state():
    return hp.oracle_state(wl=0.3, wr=0.5, goal=SR.FAR)


def _base_normals(seed, step, k, mask=()):
    """(z1, z2) [len(k), H] of oracle.dmath.noise_block with the words named in `mask` ("seed", "n",
    "k") cut to their low 32 bits: what a generator that kept the word in 32 bits would draw."""
    seed, k = int(seed) & M64, np.asarray(k, np.int64)
    if "seed" in mask:
        seed &= M32
    if "k" in mask:
        k = k & np.int64(M32)
    z1, z2 = np.empty((k.size, H), F32), np.empty((k.size, H), F32)
    for tp in range(NB):
        n = (int(step) * NB + tp) & M64
        if "n" in mask:
            n &= M32
        b = dmath.noise_block(seed, n, k)
        for j, t in enumerate(range(2 * tp, min(2 * tp + 2, H))):
            z1[:, t], z2[:, t] = b[2 * j], b[2 * j + 1]
    return z1, z2


def _differs(a, b):
    """[rows, H] bool: where either normal of two draws differs."""
    return (a[0].view(np.uint32) != b[0].view(np.uint32)) | (a[1].view(np.uint32) != b[1].view(np.uint32))


def _wide_words_matter(seed, step, k):
    """The preconditions on the normals of one step at the source indices k; returns the words that are wide."""
    seed, step = int(seed) & M64, int(step)
    true = _base_normals(seed, step, k)
    full = dmath.noise(seed, step, k, H)             # (the masking helper with no mask is the oracle's noise)
    assert not _differs(true, full).any()
    wide = []
    if seed >> 32:
        wide.append("seed")
        assert _differs(true, _base_normals(seed, step, k, ("seed",))).any(axis=1).all(), "the seed's high word is idle"
    if (k >> 32).any():
        wide.append("k")
        d = _differs(true, _base_normals(seed, step, k, ("k",)))
        above = (k >> 32) != 0
        assert not d[~above].any() and d[above].any(axis=1).all(), "the trajectory index's high word is idle"
    n = [(step * NB + tp) & M64 for tp in range(NB)]
    if any(x >> 32 for x in n):
        wide.append("n")
        d = _differs(true, _base_normals(seed, step, k, ("n",)))
        cols = np.repeat([x >> 32 != 0 for x in n], 2)[:H]
        assert not d[:, ~cols].any() and d[:, cols].all(axis=0).all() and d[:, cols].any(axis=1).all(), \
            "the block index's high word is idle"
    return wide


def _expected(p, st, u1n, u2n, step, plan, k_offset):
    """The oracle's step on the controls sampled at (p.seed, step, k_offset ..) under `plan`, preconditions asserted."""
    k = np.arange(k_offset, k_offset + p.K, dtype=np.int64)
    src, _, _ = S.plan_sources(k, plan)
    wide = _wide_words_matter(p.seed, step, np.unique(src))
    u1, u2 = SR.controls(p, st, u1n, u2n, step, plan, k_begin=k_offset)
    inside = ((u1 > p.f("min_u1")) & (u1 < p.f("max_u1"))).mean(), ((u2 > p.f("min_u2")) & (u2 < p.f("max_u2"))).mean()
    assert min(inside) >= 0.99, f"clamped samples hide their normals: {inside}"
    out = R.mppi_step(p, _scene(), st, u1n, u2n, 0, "3d", injected=(u1, u2))      # (injected: the step is not read)
    for name in ("cost",) + tuple(b for _, b in SR.OUT_KEYS):
        assert np.isfinite(out[name]).all(), f"the oracle's {name} is not finite"
    out["u1"], out["u2"], out["wide"] = u1, u2, wide
    return out


@functools.lru_cache(maxsize=None)
def _one_step(plan, seed, k_offset, step, K=300):
    """One step from a fixed non-zero nominal sequence (so the nominal row of a plan is not all zero)."""
    p = R.Params(K=K, H=H, seed=int(seed) & M64)
    u1n = np.linspace(0.05, 0.2, H).astype(F32)
    u2n = np.linspace(-0.2, 0.1, H).astype(F32)
    return p, u1n, u2n, _expected(p, _state(), u1n, u2n, step, PLANS[plan], k_offset)


@functools.lru_cache(maxsize=None)
def _loop(K, seed, plan, steps, k_offset=0):
    """The closed loop over the step numbers `steps` from u_nom = 0, nominal sequence and state fed back
    (sampling_refs.closed_loop with the step numbers given): a list of (state, u_nom1, u_nom2, out)."""
    p = R.Params(K=K, H=H, seed=int(seed) & M64, **LOOP_BOUNDS)
    st, u1, u2 = _state(), np.zeros(H, F32), np.zeros(H, F32)
    rows, wide = [], set()
    for step in steps:
        out = _expected(p, st, u1, u2, step, PLANS[plan], k_offset)
        wide.update(out["wide"])
        rows.append((st, u1, u2, out))
        u1, u2 = out["u1_opt"], out["u2_opt"]
        st = SR.next_state(st, out, p)
    assert "n" in wide and "seed" in wide, wide
    return rows


# ------------------------------------------------------------------ engines
def _engine(K, seed, k_offset, plan, mode, monkeypatch, **params):
    """mode: "roles" / "pair" (separate launches on either rollout kernel) or "server"."""
    if mode == "server":
        monkeypatch.delenv("MPPI_ROLES", raising=False)
    else:
        monkeypatch.setenv("MPPI_ROLES", "1" if mode == "roles" else "0")
    eng = SR.engine(K, H, seed, PLANS[plan], k_offset=k_offset, **params)
    try:
        if mode == "server":
            eng.set_option("resident", 2)
            eng.set_option("resident_idle_us", 100000)
        else:
            eng.set_option("resident", 0)
    except BaseException:
        eng.close()
        raise
    return eng


def _separate(info, mode):
    """Separate launches on the rollout kernel the mode names: the role-split kernel's workgroup is four
    waves per trajectory wave (1024 threads), the pair kernel's two (512)."""
    assert info["resident"] == 0 and info["server_steps"] == 0, info
    assert info["block"] == (1024 if mode == "roles" else 512), (mode, info)


def _same_dump(eng, want, tag):
    d = eng.dump()
    for k in ("u1", "u2"):
        assert np.array_equal(d[k].view(np.uint32), want[k].view(np.uint32)), f"{tag}: " + hp.mismatch_report(k, d[k], want[k])


# ------------------------------------------------------------------ a. each word, each generator form
# (the case list and its coverage: tests/wide_key_cases.py, checked on the CPU by tests/test_step_word.py)
@pytest.mark.parametrize("mode", ["roles", "pair"])
@pytest.mark.parametrize("case", CASES, ids=WK.case_id)
def test_one_step_equals_oracle(case, mode, monkeypatch):
    """The first step of a fresh context (so step 2^64 - 1 meets empty normals slots), separate launches."""
    plan, seed, k_offset, step = case
    p, u1n, u2n, want = _one_step(plan, seed, k_offset, step)
    assert want["wide"], case
    tag = f"{WK.case_id(case)} {mode}"
    eng = _engine(p.K, seed, k_offset, plan, mode, monkeypatch)
    try:
        assert int(eng.params.seed) == p.seed            # (seed -1 arrives as 2^64 - 1)
        eng.set_nominal(u1n, u2n)
        eng.step("3d", step, copy=False)
        SR.same_step(eng.outputs(), eng.costs(), want, tag)
        _same_dump(eng, want, tag)
        _separate(eng.launch_info(), mode)
    finally:
        eng.close()


# ------------------------------------------------------------------ b. step sequences over the edges
SEQUENCES = {
    "2^32 inside a step": tuple(range(S0 - 2, S0 + 4)),
    "2^63": tuple(range(2 ** 63 - 3, 2 ** 63 + 3)),
    "wrap": (2 ** 64 - 3, 2 ** 64 - 2, 2 ** 64 - 1, 0, 1),
    "jumps": (0, 2 ** 64 - 1, 2 ** 64 - 1, 5, 2 ** 63, 2 ** 63 + 1),
}


def _drive(eng, rows, steps, tag):
    for (st, _, _, want), step in zip(rows, steps):
        eng.set_state(hp.state_for(st))
        eng.step("3d", step, copy=False)
        SR.same_step(eng.outputs(), eng.costs(), want, f"{tag} step {step:#x}")
    _same_dump(eng, rows[-1][3], tag)


def _served(info, n_steps):
    """A shape that fell back to separate launches must not pass."""
    assert info["resident"] == 1 and info["server_steps"] == n_steps, info
    assert info["server_failed_steps"] == 0 and info["server_fallbacks"] == 0, info


def _noise_phase_rule(info):
    """server_step's rule for generating step + 2 in the server's own noise phase."""
    spare = info["blocks"] - info["finish_groups"]
    return spare >= 2 and 4 * spare >= info["blocks"]


@pytest.mark.parametrize("mode", ["roles", "pair", "server"])
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_step_sequences_in_closed_loop(name, mode, monkeypatch):
    """K = 768 (three records): on the server the noise kernel generates step + 2 beside the step."""
    steps = SEQUENCES[name]
    rows = _loop(768, GOLDEN, "default", steps)
    eng = _engine(768, GOLDEN, 0, "default", mode, monkeypatch, **LOOP_BOUNDS)
    try:
        _drive(eng, rows, steps, f"{name} {mode}")
        info = eng.launch_info()
        if mode == "server":
            _served(info, len(steps))
            assert not _noise_phase_rule(info), info
            assert info["block"] == 1024, info
        else:
            _separate(info, mode)
    finally:
        eng.close()


@pytest.mark.parametrize("name,plan", [("2^32 inside a step", "default"), ("2^32 inside a step", "anti"),
                                       ("wrap", "default"), ("2^63", "anti"), ("jumps", "default")])
def test_server_noise_phase_carries_the_block_index(name, plan, monkeypatch):
    """K = 4096, H = 5: 16 records, E = 12, two columns a finish group, 6 groups, so 10 workgroups are
    spare and the server's noise phase draws step + 2 from the command's noise_n_base_lo / _hi: over
    the sequence (step + 2) * 3 carries from the low word into the high one, leaves the signed range
    and wraps.  Without a plan and with one (both forms of the phase's generator).  "jumps": a step no
    slot holds stops the server before a slot its noise phase may still be writing is regenerated."""
    steps = SEQUENCES[name]
    rows = _loop(4096, GOLDEN, plan, steps)
    eng = _engine(4096, GOLDEN, 0, plan, "server", monkeypatch, **LOOP_BOUNDS)
    try:
        _drive(eng, rows, steps, f"{name} {plan} noise phase")
        info = eng.launch_info()
        _served(info, len(steps))
        assert info["blocks"] == 16 and _noise_phase_rule(info), info
    finally:
        eng.close()


# ------------------------------------------------------------------ c. batch
BATCH_K, BATCH_STEPS = 256, 4
BATCH_SEEDS = (2 ** 32, GOLDEN, 2 ** 64 - 1)
# The batch picks its noise kernel by whether any sampling row or a context plan exists
# (launch_batch_noise), and the plan kernel its generator by the episode's plan:
#   "plain"  no sampling row, default context plan: mppi_batch_noise_kernel
#   "plans"  mppi_batch_noise_plan_kernel: an SR.ANTI row (the elementwise generator), an episode
#            without a row (the plain generator inside the plan kernel) and an SR.ALL row (the serial one)
BATCH_PLANS = dict(plain=("default", "default", "default"), plans=("anti", "default", "all"))
AHEAD = (1.0, 0.0, 0.0)


def _start():
    return B.start_state(B.START, SR.FAR, AHEAD)


@functools.lru_cache(maxsize=None)
def _episode_ref(seed, plan):
    """Reference A of one episode, SR.oracle_loop with the closed loops' control bounds.  The same loop
    is then walked step by step through _expected, which asserts the preconditions of every step (the
    seed's high word changes every row's normals, 99 % of the samples unclamped, finite costs) and must
    reproduce the reference's rows."""
    seed &= M64
    assert seed >> 32
    ref = SR.oracle_loop(BATCH_K, H, _start(), seed, BATCH_STEPS, PLANS[plan], params=R.Params(**LOOP_BOUNDS))
    assert ref["steps"] == BATCH_STEPS and np.isfinite(ref["rows"]).all()
    p = R.Params(K=BATCH_K, H=H, seed=seed, **LOOP_BOUNDS)
    st, u1, u2 = _start(), np.zeros(H, F32), np.zeros(H, F32)
    for i in range(BATCH_STEPS):
        s = R.State(x=float(st["x"]), y=float(st["y"]), heading=np.asarray(st["heading"], np.float64),
                    left_wheel_speed=float(st["wl"]), right_wheel_speed=float(st["wr"]), goal_x=float(st["gx"]),
                    goal_y=float(st["gy"]), std_dev_u1=float(st["s1"]), std_dev_u2=float(st["s2"]))
        o = _expected(p, s, u1, u2, i, PLANS[plan], 0)
        assert o["wide"] == ["seed"]
        u1, u2 = o["u1_opt"], o["u2_opt"]
        st, row = B.rule(st, o["traj_sim"][0], o["hv_sim"][0], o["v_opt"][0], o["w_opt"][0], p.robot_radius, B.RUN)
        assert np.array_equal(np.asarray(row, F32).view(np.uint32), ref["rows"][i].view(np.uint32)), (hex(seed), plan, i)
    low = SR.oracle_loop(BATCH_K, H, _start(), seed & M32, BATCH_STEPS, PLANS[plan], params=R.Params(**LOOP_BOUNDS))
    assert V.differ(ref, low) == BATCH_STEPS, "the seed's high word is idle"
    return ref


def _rows(config):
    """(variant rows, plan name -> row index) of a configuration: one sampling row per plan that is not the default."""
    from mppi_amd.batch import variant_dict
    names = [n for n in dict.fromkeys(BATCH_PLANS[config]) if n != "default"]
    rows = [dict(variant_dict("3d"), antithetic=PLANS[n]["antithetic"], nominal=PLANS[n]["nominal"],
                 noise_beta=PLANS[n]["beta"]) for n in names]
    return rows, {n: i for i, n in enumerate(names)}


def _open_batch(config, seeds=None):
    """(engine, batch, plan name -> variant index): E = 3 on a context that never had a plan set; "plain"
    sets no variant at all, so the batch has no sampling row."""
    from mppi_amd import _lib
    eng = V.make_engine(BATCH_K, H, seed=42, **LOOP_BOUNDS)
    try:
        batch = _lib.Batch(eng, 3)
        rows, index = _rows(config)
        if rows:
            batch.set_variants(rows)
        if seeds is not None:
            for e, (seed, plan) in enumerate(zip(seeds, BATCH_PLANS[config])):
                batch.set_episode(e, V.mppi_state(_start()), seed, index.get(plan, -1))
    except BaseException:
        eng.close()
        raise
    return eng, batch, index


@pytest.mark.parametrize("config", list(BATCH_PLANS))
def test_batch_episode_seeds(config):
    from mppi_amd import _lib
    eng, batch, _ = _open_batch(config, BATCH_SEEDS)
    try:
        batch.run(BATCH_STEPS, "3d", _lib.make_policy(**B.RUN))
        for e, (seed, plan) in enumerate(zip(BATCH_SEEDS, BATCH_PLANS[config])):
            V.same(V.collect(batch, e), _episode_ref(seed, plan), f"{config} episode {e} seed {seed:#x} {plan}")
        batch.close()
    finally:
        eng.close()


@pytest.mark.parametrize("config", list(BATCH_PLANS))
def test_batch_task_seeds(config):
    """Every wide seed under every plan of the configuration, as tasks on the three lanes."""
    from mppi_amd import _lib
    tasks = [(seed, plan) for plan in dict.fromkeys(BATCH_PLANS[config]) for seed in BATCH_SEEDS]
    eng, batch, index = _open_batch(config)
    try:
        batch.set_tasks([_lib.make_task(V.mppi_state(_start()), seed, BATCH_STEPS, index.get(plan, -1))
                         for seed, plan in tasks])
        done = 0
        while done < len(tasks):
            done, steps = batch.run_tasks(100, "3d", _lib.make_policy(**B.RUN))
            assert steps > 0 or done == len(tasks)
        for i, (seed, plan) in enumerate(tasks):
            ref = _episode_ref(seed, plan)
            assert batch.task(i)["steps"] == ref["steps"], (i, seed, plan)
            assert np.array_equal(batch.task_log(i).view(np.uint32), ref["rows"].view(np.uint32)), (i, hex(seed), plan)
        batch.close()
    finally:
        eng.close()


@pytest.mark.parametrize("config", list(BATCH_PLANS))
@pytest.mark.parametrize("dtype,words", [("uint64", BATCH_SEEDS), ("int64", (2 ** 32, -2 ** 63, -1))])
def test_batch_step_device_reseeds(dtype, words, config):
    """Episodes set with narrow seeds take two steps, then are reset with the wide seeds from a device
    tensor (uint64 words as they are; int64 -1 and -2^63 are the keys 2^64 - 1 and 2^63) and run the
    closed loop of the fresh episode with that key."""
    import torch
    from mppi_amd.batch import advance_state, pack_states, state_dict
    E, plans = 3, BATCH_PLANS[config]
    start = state_dict(B.START[0], B.START[1], AHEAD, 0.0, 0.0, SR.FAR[0], SR.FAR[1], 0.25, 0.25)
    refs = [_episode_ref(w & M64, plan) for w, plan in zip(words, plans)]
    seeds = torch.as_tensor(np.array(words, dtype=dtype)).cuda()
    reset = torch.ones(E, dtype=torch.int32).cuda()
    eng, batch, _ = _open_batch(config, (5, 6, 7))
    try:
        radius = float(eng.params.robot_radius)

        def step(states, **kw):
            cmd, plan = batch.step_device(torch.as_tensor(pack_states(states)).cuda(), **kw)
            eng.sync()
            cmd, plan = cmd.cpu().numpy(), plan.cpu().numpy()
            out = [advance_state(states[e], plan[e, 4 * H:4 * H + 3], plan[e, 4 * H + 3:4 * H + 6], cmd[e, 0],
                                 cmd[e, 1], radius, B.RUN) for e in range(E)]
            return [s for s, _ in out], [r for _, r in out]

        states = [dict(start) for _ in range(E)]
        for _ in range(2):
            states, _ = step(states)
        states, rows = [dict(start) for _ in range(E)], [[] for _ in range(E)]
        for i in range(BATCH_STEPS):
            states, new = step(states, **(dict(reset=reset, seeds=seeds) if i == 0 else {}))
            for e in range(E):
                rows[e].append(new[e])
        for e in range(E):
            got = np.array(rows[e], F32)
            assert np.array_equal(got.view(np.uint32), refs[e]["rows"].view(np.uint32)), (dtype, e, hex(words[e] & M64))
            assert batch.episode(e)["steps_total"] == BATCH_STEPS
        batch.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ d. group
def test_group_members_meet_at_2_32():
    """Two members of 256 on device 0 with the context's k_offset = 2^32 - 256: member 0 ends at 2^32,
    member 1 starts there.  Two steps from step 2^40, bitwise the one context and the oracle."""
    from mppi_amd import _lib
    K, k_offset, seed, steps = 512, 2 ** 32 - 256, 2, (2 ** 40, 2 ** 40 + 1)
    st, p = _state(), R.Params(K=K, H=H, seed=seed)
    Z, hw, cm = hp.c3_scene()
    one = SR.engine(K, H, seed, k_offset=k_offset)
    g = None
    try:
        g = _lib.Group(_lib.make_params(K, H, k_offset=k_offset, seed=seed), [0, 0])
        g.set_dem(Z, hw)
        g.set_costmap(cm, hw)
        g.set_state(hp.state_for(st))
        assert [g.shard(i) for i in range(2)] == [(0, 256), (256, 256)]
        assert [int(m.params.k_offset) for m in g.members] == [2 ** 32 - 256, 2 ** 32]
        u1n, u2n = np.zeros(H, F32), np.zeros(H, F32)
        for step in steps:
            want = _expected(p, st, u1n, u2n, step, SR.DEFAULT, k_offset)
            assert want["wide"] == ["k", "n"]
            a, b = g.step("3d", step), one.step("3d", step)
            for k in a:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (hex(step), k)
            assert np.array_equal(g.costs().view(np.uint32), one.costs().view(np.uint32))
            SR.same_step(a, g.costs(), want, f"group step {step:#x}")
            SR.same_step(b, one.costs(), want, f"one context step {step:#x}")
            _same_dump(one, want, f"one context step {step:#x}")
            u1n, u2n = want["u1_opt"], want["u2_opt"]
    finally:
        if g is not None:
            g.close()
        one.close()
