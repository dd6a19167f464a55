"""GPU: crater-field DEMs built on the device (mppi_dem_builder_* / mppi_build_dem / mppi_batch_build_dem,
csrc/mppi_dem_build.hip).

The product kernel's lane maps are pinned with exact integer factors; built terrains are compared with the
reference's own Surface.create_surface output (tests/golden/crater_fields.npz) by the rule of
tests/crater_helpers.py (every cell within one float32 ulp, at most 1e-3 of the cells differing at all);
an engine or a batch slot built on the device steps bitwise as one given the same heights by set_dem.
"""
import ctypes as C

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V
from crater_helpers import CASE_IDS, assert_dem_close, crater_cases
from mppi_amd import scene
from oracle import mppi_ref as R

pytestmark = pytest.mark.gpu

MPPI_EINVAL, MPPI_ESTATE = -1, -3
VARIANTS = ("mfma", "valu")
N, HW, K, H = 130, 6.5, 256, 20          # the 130^2 fixture case's grid
START, FAR = (0.5, 0.5), (5.0, 4.0)      # never reached within the few steps run here


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _costmap():
    x = np.linspace(-HW, HW, 16)
    X, Y = np.meshgrid(x, -x)
    return (0.8 * np.exp(-((X - 2.0) ** 2 + (Y - 1.5) ** 2) / 2.0)).astype(np.float32)


def _fields():
    """Three crater lists on the 130^2 grid: the fixture's, and two more from its generator's recipe."""
    rng = np.random.RandomState(17)
    more = [np.stack([rng.uniform(-HW, HW, n), rng.uniform(-HW, HW, n), rng.uniform(0.6, 4.5, n),
                      rng.uniform(0.5, 3.0, n)], 1) for n in (5, 2)]
    return [crater_cases()[1][2]] + more


def _engine(seed=42):
    from mppi_amd import _lib
    return _lib.Engine(_lib.make_params(K, H, seed=seed), 0)


# ---- 1. the product kernel's lane maps, exact ----
def _int_factors(grid, terms, skew):
    i = np.arange(grid, dtype=np.float64)
    t = np.arange(terms, dtype=np.float64)
    Rm = np.repeat((i + 1)[:, None], terms, 1) + skew * t[None, :]        # R[i][t]
    Cm = (t + 1)[:, None] * (i + 1)[None, :]                               # C[t][j]
    return Rm, Cm


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("grid,terms,skew", [(17, 8, 0), (130, 12, 0), (130, 12, 3), (67, 40, 3)],
                         ids=["17x8", "130x12", "130x12-skewed", "67x40-two-chunks"])
def test_product_lane_map_is_exact(grid, terms, skew, variant):
    """R[i][t] = i + 1 (+ skew t), C[t][j] = (t + 1)(j + 1): every entry of the product is an exact integer
    below 2^24, so the float32 output is the integer product bit for bit.  A result in the wrong row (the
    f32 C/D row formula on the f64 MFMA) or a row/column swap (the skewed case is not symmetric) fails."""
    torch = _gpu()
    from mppi_amd import _lib
    Rm, Cm = _int_factors(grid, terms, skew)
    want = Rm @ Cm
    assert want.max() < 2 ** 24 and np.array_equal(want, np.round(want))
    if skew:
        assert not np.array_equal(want, want.T)
    r_dev = torch.from_numpy(np.ascontiguousarray(Rm.T)).cuda()     # term-major [terms][grid]
    c_dev = torch.from_numpy(np.ascontiguousarray(Cm)).cuda()
    torch.cuda.synchronize()
    b = _lib.DemBuilder(0)
    try:
        got = b.product(r_dev.data_ptr(), c_dev.data_ptr(), terms, grid, variant=variant)
    finally:
        b.close()
    bad = np.argwhere(got != want.astype(np.float32))
    assert bad.size == 0, f"{len(bad)} wrong entries, first at {bad[0]}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


# ---- 2. the fixture ----
@pytest.mark.parametrize("case", range(4), ids=CASE_IDS)
def test_builder_matches_the_reference(case):
    torch = _gpu()
    from mppi_amd import _lib
    grid, hw, craters, ref = crater_cases()[case]
    b = _lib.DemBuilder(0)
    try:
        got = {v: b.build(craters, grid, hw, variant=v) for v in VARIANTS}
        assert b.last_ms() > 0.0
        nested = [((r[0], r[1]), r[2], r[3]) for r in craters.tolist()]      # the reference's own list shape
        assert np.array_equal(b.build(nested, grid, hw).view(np.uint32), got["mfma"].view(np.uint32))
        out = torch.full((grid, grid), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert b.build(craters, grid, hw, out_device=out.data_ptr()) is None
        assert np.array_equal(out.cpu().numpy().view(np.uint32), got["mfma"].view(np.uint32))
    finally:
        b.close()
    for v in VARIANTS:
        assert_dem_close(got[v], ref, f"{CASE_IDS[case]} {v} vs the reference")
    assert_dem_close(got["mfma"], got["valu"], f"{CASE_IDS[case]} mfma vs valu")


# ---- 3. edges ----
@pytest.mark.parametrize("variant", VARIANTS)
def test_no_crater_gives_the_base_or_zeros(variant):
    _gpu()
    from mppi_amd import _lib
    base = (np.float32(1e-3) * np.arange(N * N, dtype=np.float32)).reshape(N, N) - np.float32(3.0)
    eng = _engine()
    b = _lib.DemBuilder(0)
    try:
        got = eng.build_dem([], N, HW, base=base, variant=variant)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
        assert eng.dem_shape == (N, N)
        zeros = b.build(np.zeros((0, 4)), 17, 0.85, variant=variant)
        assert zeros.shape == (17, 17) and not zeros.view(np.uint32).any()
    finally:
        b.close()
        eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_base_outside_and_narrow_craters(variant):
    """A base added before the one rounding; a crater centred at 3 hw (outside the map, not culled); one of
    width 0.01 (its factors underflow to 0 a few cells from the centre), placed on a grid point."""
    _gpu()
    from mppi_amd import _lib
    x = np.linspace(-HW, HW, N)
    base = (np.float32(1e-3) * np.arange(N * N, dtype=np.float32)).reshape(N, N)
    cases = [("base", crater_cases()[1][2], base),
             ("outside", [((3 * HW, 0.4), 4.0, 9.0), ((-1.0, 2.0), 2.0, 1.5)], None),
             ("narrow", [((x[40], x[77]), 3.0, 0.01)], None)]
    b = _lib.DemBuilder(0)
    try:
        for name, bumps, bs in cases:
            got = b.build(bumps, N, HW, base=bs, variant=variant)
            want = scene.crater_dem_separable(N, HW, bumps, base=bs)
            assert_dem_close(got, want, f"{name} {variant}")
            if name == "narrow":   # the bowl at its grid point, zero two cells away
                assert got[77, 40] == want[77, 40] == np.float32(-1.0) and got[77, 42] == 0.0
            if name == "outside":  # the far crater's rim reaches the map's edge
                far_only = scene.crater_dem_separable(N, HW, bumps[:1])
                assert np.abs(far_only[:, -1]).max() > 1e-2
    finally:
        b.close()


# ---- 4. the engine ----
def _loop(make, steps, proj):
    return B.engine_loop(K, H, None, None, None, B.start_state(START, FAR), 42, steps, proj, make_engine=make)


def test_engine_build_dem_then_steps():
    """Engine.build_dem leaves the geometry, the normal table and the reciprocal of set_dem: 3 steps in 3D
    and 1 in 2D are bitwise the oracle's on the returned heights and a second engine's after set_dem."""
    torch = _gpu()
    craters = crater_cases()[1][2]
    cm = _costmap()
    built = {}

    def make_built(seed):
        eng = _engine(seed)
        built["Z"] = eng.build_dem(craters, N, HW)
        eng.set_costmap(cm, HW)
        return eng

    def make_set(seed):
        eng = _engine(seed)
        eng.set_dem(built["Z"], HW)
        eng.set_costmap(cm, HW)
        return eng

    keep = {}

    def make_borrowed_then_built(seed):
        eng = _engine(seed)
        t = keep["t"] = torch.full((N, N), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.set_dem_device(t.data_ptr(), N, N, HW, keepalive=t)
        Z = eng.build_dem(craters, N, HW, variant="valu", copy_out=True)
        assert_dem_close(Z, built["Z"], "valu vs mfma in the engine")
        eng.build_dem(craters, N, HW, copy_out=False)
        eng.set_costmap(cm, HW)
        return eng

    for proj, steps in (("3d", 3), ("2d", 1)):
        got = _loop(make_built, steps, proj)
        assert got["steps"] == steps
        assert_dem_close(built["Z"], crater_cases()[1][3], "engine heights vs the reference")
        want = B.oracle_loop(K, H, R.Scene(built["Z"], HW, cm), B.start_state(START, FAR), 42, steps, proj)
        V.same(got, want, f"{proj}: built vs the oracle")
        V.same(got, _loop(make_set, steps, proj), f"{proj}: built vs set_dem")
        V.same(got, _loop(make_borrowed_then_built, steps, proj), f"{proj}: built over a borrowed DEM")
        assert bool((keep["t"] == 7.0).all()), "the borrowed DEM was written into"
    flat = B.oracle_loop(K, H, R.Scene(np.zeros((N, N), np.float32), HW, cm), B.start_state(START, FAR), 42, 3, "3d")
    assert V.differ(_loop(make_built, 3, "3d"), flat) >= 1      # the terrain acts on the loop


# ---- 5. the batch ----
SLOTS = (0, 7, 255)


def _batch_run(fill, runs, refill):
    """Six episodes over three DEM slots; fill(batch, slot, i) fills slot with field i; refill is applied
    before the second run.  Returns the episodes' results with the rows of both runs."""
    from mppi_amd import _lib
    eng = _engine()
    try:
        eng.set_dem(np.zeros((N, N), np.float32), HW)
        eng.set_costmap(_costmap(), HW)
        batch = _lib.Batch(eng, 6)
        for i, s in enumerate(SLOTS):
            fill(batch, s, i)
        for e in range(6):
            batch.set_episode(e, V.mppi_state(B.start_state(START, FAR)), 100 + e, dem=SLOTS[e % 3])
        logs = [[] for _ in range(6)]
        for r, n in enumerate(runs):
            if r:
                refill(batch)
            batch.run(n, "3d", _lib.make_policy(**B.RUN))
            for e in range(6):
                logs[e].append(batch.log(e))
        out = []
        for e in range(6):
            res = V.collect(batch, e)
            res["rows"] = np.concatenate(logs[e])
            res["steps"] = len(res["rows"])
            out.append(res)
        batch.close()
    finally:
        eng.close()
    return out


def test_batch_build_dem_slots():
    """Three slots built from three crater lists, six episodes over them, a slot rebuilt between two runs:
    logs, final states and step counts are bitwise those of a batch whose slots got the same heights by
    set_dem."""
    _gpu()
    fields = _fields()
    heights = {}

    def build(batch, slot, i, key=None, variant="mfma"):
        heights[i if key is None else key] = batch.build_dem(slot, fields[i], HW, copy_out=True, variant=variant)

    got = _batch_run(build, (4, 4), lambda batch: build(batch, SLOTS[1], 2, "again", "valu"))
    assert_dem_close(heights[0], crater_cases()[1][3], "slot 0 vs the reference")
    for i in range(3):
        assert_dem_close(heights[i], scene.crater_dem_separable(N, HW, fields[i]), f"slot {i} vs separable")
    assert_dem_close(heights["again"], heights[2], "valu vs mfma")
    want = _batch_run(lambda batch, slot, i: batch.set_dem(slot, heights[i]), (4, 4),
                      lambda batch: batch.set_dem(SLOTS[1], heights["again"]))
    for e in range(6):
        V.same(got[e], want[e], f"episode {e}")
        assert got[e]["steps"] == 8
    never = _batch_run(lambda batch, slot, i: batch.set_dem(slot, heights[i]), (4, 4), lambda batch: None)
    assert V.differ(want[1], never[1]) >= 1 and V.differ(want[0], never[0]) == 0     # the rebuilt slot acts


def test_run_campaign_takes_crater_fields():
    """run_campaign(dems=[CraterField, array, CraterField]) gives what arrays alone give."""
    _gpu()
    from mppi_amd import _lib, controller
    fields = _fields()
    b = _lib.DemBuilder(0)
    arrays = [b.build(f, N, HW) for f in fields]
    b.close()
    cfg = controller._load_config(controller.DEFAULT_CONFIG)
    cfg = {**cfg, "controller": {**cfg["controller"], "number_of_trajectories": K, "number_of_iterations": H},
           "engine": {**(cfg.get("engine") or {}), "seed": 11}}
    res = []
    for dems in ([scene.CraterField(fields[0]), arrays[1], scene.CraterField(fields[2])], arrays):
        surface = controller.Surface.from_arrays(np.zeros((N, N), np.float32), _costmap(), HW, radius_robot=0.3)
        robot = controller.Robot(START[0], START[1], [1.0, 0.0, 0.0], cfg)
        ctl = controller.MPPI_Controller(surface, robot, cfg, FAR[0], FAR[1], 0.0)
        ctl.std_dev_u1 = ctl.std_dev_u2 = 0.25
        res.append(ctl.run_campaign([START] * 4, [(1.0, 0.0, 0.0)] * 4, [FAR] * 4, seeds=[5, 6, 7, 8], lanes=2,
                                    max_loops=[3, 5, 4, 3], dems=dems, task_dem=[0, 1, 2, -1]))
        ctl.engine.close()
    for i, (a, w) in enumerate(zip(*res)):
        assert a["loops"] == w["loops"] == [3, 5, 4, 3][i]
        for key in ("x", "y", "z", "lin_vel", "ang_vel"):
            assert np.array_equal(np.asarray(a[key], np.float32).view(np.uint32),
                                  np.asarray(w[key], np.float32).view(np.uint32)), (i, key)
    assert res[0][0]["z"] != res[0][3]["z"]      # a built slot is not the controller's flat surface


def test_surface_dem_builder_device():
    """Surface.dem_builder = "device": create_surface returns the builder's heights; the default stays
    the host path."""
    _gpu()
    from mppi_amd import controller
    assert controller.Surface.dem_builder == "host"
    s = controller.Surface.__new__(controller.Surface)
    s.grid_size, s.half_width = N, HW
    bumps = [((r[0], r[1]), r[2], r[3]) for r in crater_cases()[1][2].tolist()]
    _, _, host = s.create_surface(bumps)
    assert np.array_equal(host, scene.crater_dem(N, HW, bumps).astype(np.float64))
    s.dem_builder = "device"
    X, Y, dev = s.create_surface(bumps)
    assert dev.dtype == np.float64 and X.shape == Y.shape == dev.shape == (N, N)
    assert_dem_close(dev.astype(np.float32), crater_cases()[1][3], "Surface device builder")
    s._dem_builder.close()


# ---- 6. refusals ----
def test_refusals():
    """Every refused call returns its code and names what is wrong, and leaves engine and batch usable."""
    _gpu()
    from mppi_amd import _lib
    lib = _lib.load_library()
    craters = np.ascontiguousarray(crater_cases()[1][2])
    cp = craters.ctypes.data_as(_lib._DP)
    out = np.empty((N, N), np.float32)

    def refused(rc, *words, code=MPPI_EINVAL):
        assert rc == code, (rc, lib.mppi_last_error())
        msg = lib.mppi_last_error()
        for w in words:
            assert w.encode() in msg, (w, msg)

    def bad(k, f, v):
        c = craters.copy()
        c[k, f] = v
        return c

    b = _lib.DemBuilder(0)
    eng = _engine()
    try:
        # null arguments; a crater list that is not (n, 4)
        refused(lib.mppi_dem_builder_create(0, None), "null")
        refused(lib.mppi_dem_builder_build(None, cp, 3, N, HW, None, _lib._fp(out), None, 0), "null")
        refused(lib.mppi_dem_builder_build(b.h, None, 3, N, HW, None, _lib._fp(out), None, 0), "craters", "null")
        refused(lib.mppi_dem_builder_last_ms(b.h, None), "null")
        refused(lib.mppi_build_dem(None, cp, 3, N, HW, None, None, 0), "null")
        refused(lib.mppi_batch_build_dem(None, 0, cp, 3, HW, None, None, 0), "null")
        refused(lib.mppi_dem_builder_product(b.h, None, None, 8, 17, _lib._fp(out), None, 0), "null")
        refused(lib.mppi_dem_builder_product(b.h, None, None, 6, 17, _lib._fp(out), None, 0), "multiple of 4")
        with pytest.raises(ValueError):
            b.build(np.zeros((2, 3)), N, HW)
        with pytest.raises(ValueError):
            b.build(craters, N, HW, base=np.zeros((N, N - 1), np.float32))
        with pytest.raises(ValueError):
            b.build(craters, N, HW, variant="tensor")
        # the argument checks, through each of the three forms
        for call in (lambda c, n, g, hw, v=0: lib.mppi_dem_builder_build(b.h, c.ctypes.data_as(_lib._DP), n, g, hw, None,
                                                                         _lib._fp(out), None, v),
                     lambda c, n, g, hw, v=0: lib.mppi_build_dem(eng.ctx, c.ctypes.data_as(_lib._DP), n, g, hw, None,
                                                                 None, v)):
            refused(call(craters, -1, N, HW), "n must be >= 0")
            refused(call(bad(1, 0, np.nan), 3, N, HW), "crater 1", "cx")
            refused(call(bad(2, 1, np.inf), 3, N, HW), "crater 2", "cy")
            refused(call(bad(0, 2, -np.inf), 3, N, HW), "crater 0", "height")
            refused(call(bad(1, 3, np.nan), 3, N, HW), "crater 1", "width")
            refused(call(bad(2, 3, 0.0), 3, N, HW), "crater 2", "width", "non-zero")
            refused(call(craters, 3, 1, HW), "grid_size")
            refused(call(craters, 3, N, 0.0), "half_width")
            refused(call(craters, 3, N, np.inf), "half_width")
            refused(call(craters, 3, N, HW, 2), "variant")
        # a refused build leaves the engine without a DEM, as before
        eng.set_costmap(_costmap(), HW)
        batch = _lib.Batch(eng, 2)
        refused(lib.mppi_batch_build_dem(batch.h, 0, cp, 3, HW, None, None, 0), "no DEM", code=MPPI_ESTATE)
        # the context's DEM must be square and centred with the builder's resolution
        eng.set_dem(np.zeros((N, N + 2), np.float32), HW)
        refused(lib.mppi_batch_build_dem(batch.h, 0, cp, 3, HW, None, None, 0), "not square")
        eng.set_dem(np.zeros((N, N), np.float32), HW, x_min=-HW + 1.0)
        refused(lib.mppi_batch_build_dem(batch.h, 0, cp, 3, HW, None, None, 0), "not centred")
        eng.set_dem(np.zeros((N, N), np.float32), HW, resolution=0.2)
        refused(lib.mppi_batch_build_dem(batch.h, 0, cp, 3, HW, None, None, 0), "resolution")
        eng.set_dem(np.zeros((N, N), np.float32), HW)
        refused(lib.mppi_batch_build_dem(batch.h, 0, cp, 3, 2 * HW, None, None, 0), "not centred")
        # slot out of range; the crater checks
        refused(lib.mppi_batch_build_dem(batch.h, 256, cp, 3, HW, None, None, 0), "DEM slot 256")
        refused(lib.mppi_batch_build_dem(batch.h, -1, cp, 3, HW, None, None, 0), "DEM slot -1")
        refused(lib.mppi_batch_build_dem(batch.h, 0, bad(1, 3, 0.0).ctypes.data_as(_lib._DP), 3, HW, None, None, 0),
                "crater 1", "width")
        refused(lib.mppi_batch_build_dem(batch.h, 0, cp, 3, HW, None, None, 5), "variant")
        refused(lib.mppi_batch_set_episode_scene(batch.h, 0, 0, -1), "empty")      # the refused builds filled nothing
        # a slot an episode holds is rebuilt in place, but cannot be freed
        first = batch.build_dem(3, craters, HW, copy_out=True)
        for e in range(2):
            batch.set_episode(e, V.mppi_state(B.start_state(START, FAR)), 100 + e, dem=3 if e == 0 else -1)
        again = batch.build_dem(3, _fields()[1], HW, copy_out=True)
        assert not np.array_equal(first, again)
        refused(lib.mppi_batch_set_dem(batch.h, 3, None), "DEM slot 3", "episode 0")
        batch.run(3, "3d", _lib.make_policy(**B.RUN))
        want = B.oracle_loop(K, H, R.Scene(again, HW, _costmap()), B.start_state(START, FAR), 100, 3)
        V.same(V.collect(batch, 0), want, "episode on the rebuilt slot")
        # while a campaign is unfinished a build behaves as mppi_batch_set_dem does
        st = V.mppi_state(B.start_state(START, FAR))
        batch.set_tasks([_lib.make_task(st, 7 + i, 4, dem=3) for i in range(4)])
        done, _ = batch.run_tasks(2, "3d", _lib.make_policy(**B.RUN))
        assert done < 4
        rc_set = lib.mppi_batch_set_dem(batch.h, 9, _lib._fp(np.ascontiguousarray(first)))
        rc_build = lib.mppi_batch_build_dem(batch.h, 10, cp, 3, HW, None, None, 0)
        assert rc_build == rc_set == 0, (rc_build, rc_set, lib.mppi_last_error())
        refused(lib.mppi_batch_set_dem(batch.h, 3, None), "DEM slot 3", "task")
        while done < 4:
            done, _ = batch.run_tasks(8, "3d", _lib.make_policy(**B.RUN))
        assert all(batch.task(i)["steps"] == 4 for i in range(4))
        batch.close()
        # the engine still builds
        assert_dem_close(eng.build_dem(craters, N, HW), crater_cases()[1][3], "after the refusals")
    finally:
        b.close()
        eng.close()
