"""GPU: the hazard costmap (mppi_build_costmap_hazard / mppi_batch_build_costmap_hazard /
mppi_costmap_builder_build_hazard, csrc/mppi_costmap.hip).

Every build's mask (bit 0 H0, bit 1 H1, bit 2 rock disc) is compared bit for bit with the restatement
of tests/hazard_refs.py, and its map with hazard_refs.expected_map on the occupancy H1 | discs, the way
tests/test_gpu_costmap.py holds the rock-only build: counting, thresholds and distances are integer
work and the normalisation and power are correctly rounded on both sides, so equality is asserted.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import batch_refs as B
import batch_variant_refs as V
import hazard_refs as HR
import helpers as hp
from mppi_amd import scene
from oracle import costmap_ref as CR

pytestmark = pytest.mark.gpu

MPPI_EINVAL, MPPI_ESTATE = -1, -3
METRICS = ("chamfer", "chamfer_raster", "exact")
N, HW, SIZE, RR, POWER = 192, 75.0, 24, 1.2, 20
RES = 2.0 * HW / N
ORIGIN = (0.4, -0.7)


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _rocks(n, extent=70.0, seed=5, rmax=6.0):
    rng = np.random.RandomState(seed)
    return [[rng.uniform(-extent, extent), rng.uniform(-extent, extent), rng.uniform(0.0, rmax)] for _ in range(n)]


ROCKS = {"rocks40": _rocks(40), "none": []}


@functools.lru_cache(maxsize=None)
def crater():
    return scene.crater_dem(N, HW)


@functools.lru_cache(maxsize=None)
def crater_occupancy(deg, min_cells, inflate):
    return HR.occupancy(crater(), -HW, -HW, RES, SIZE, HW, deg, min_cells, inflate)


@functools.lru_cache(maxsize=None)
def discs(rocks):
    return CR.raster(ROCKS[rocks], ORIGIN, SIZE, HW, RR)


@pytest.fixture(scope="module")
def engine():
    _gpu()
    from mppi_amd import _lib
    eng = _lib.Engine(_lib.make_params(256, 20), 0)
    eng.set_dem(crater(), HW)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def builder():
    _gpu()
    from mppi_amd import _lib
    b = _lib.CostmapBuilder(0)
    yield b
    b.close()


def check(tag, got, mask, want, want_mask):
    assert mask.dtype == np.uint8 and np.array_equal(mask, want_mask), hp.mismatch_report(tag + " mask", mask, want_mask)
    assert got.dtype == np.float32 and np.array_equal(got, want), hp.mismatch_report(tag + " map", got, want)


# ---- 1. the crater field: limits x inflate x min_cells x metrics x rocks ----
@pytest.mark.parametrize("rocks", list(ROCKS))
@pytest.mark.parametrize("metric", METRICS)
def test_crater_field(engine, metric, rocks):
    d = discs(rocks)
    plain = engine.build_costmap(ROCKS[rocks], ORIGIN, SIZE, HW, RR, POWER, metric=metric)
    for deg in (10.0, 15.0, 20.0, 30.0):
        for inflate in (0.0, 7.0):
            for mc in (1, 3, 64, 65):
                H0, H1 = crater_occupancy(deg, mc, inflate)
                got, mask = engine.build_costmap(ROCKS[rocks], ORIGIN, SIZE, HW, RR, POWER, metric=metric,
                                                 hazard=scene.Hazard(deg, inflate, mc), return_mask=True)
                tag = f"{deg} deg inflate {inflate} min_cells {mc} {metric} {rocks}"
                check(tag, got, mask, HR.expected_map(H1 | d, POWER, metric), HR.expected_mask(H0, H1, d))
                if deg == 30.0 or mc == 65:
                    assert not H0.any(), tag                       # nothing qualifies: the rock-only map, bitwise
                    assert np.array_equal(got, plain), tag


def test_crater_fixture_counts(engine):
    for deg, n0, n1 in ((10.0, 140, 231), (15.0, 81, 160), (20.0, 23, 62), (30.0, 0, 0)):
        _, mask = engine.build_costmap([], ORIGIN, SIZE, HW, RR, POWER, hazard={"max_slope_deg": deg, "inflate": 7.0},
                                       return_mask=True)
        assert (int((mask & 1).sum()), int((mask >> 1 & 1).sum())) == (n0, n1), deg


# ---- 2. geometry and defined edges, through the builder object (any DEM placement) ----
CASES = HR.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_geometry_and_edges(builder, name):
    torch = _gpu()
    Z, x_min, y_min, res, size, hw, deg, mc, inflate = CASES[name]
    z = torch.from_numpy(np.ascontiguousarray(Z)).cuda()
    torch.cuda.synchronize()
    dem = (z.data_ptr(), Z.shape[0], Z.shape[1], x_min, y_min, res)
    rocks = _rocks(6, 0.8 * hw, 9, 0.1 * hw)
    hz = scene.Hazard(deg, inflate, mc)
    for metric in METRICS:
        for obs in (rocks, []):
            want, want_mask = HR.expected_build(Z, x_min, y_min, res, obs, ORIGIN, size, hw, RR, POWER, metric, deg, mc,
                                                inflate)
            got, mask = builder.build(obs, ORIGIN, size, hw, RR, POWER, metric=metric, dem=dem, hazard=hz,
                                      return_mask=True)
            check(f"{name} {metric} rocks {len(obs)}", got, mask, want, want_mask)
            assert builder.last_ms() > 0 and builder.hazard_count_ms() > 0
            if name in ("flat", "min65"):
                assert not (mask & 3).any()
                assert np.array_equal(got, builder.build(obs, ORIGIN, size, hw, RR, POWER, metric=metric)), name
    if name == "nonfinite":
        assert mask[0, 0] & 1 and mask[-1, -1] & 1       # the +-Inf corners' cells
    if name == "t2_160_33":
        assert HR.threshold(inflate, size, hw) == 2
    assert bool((z.cpu().numpy().view(np.uint32) == np.ascontiguousarray(Z).view(np.uint32)).all()), "the DEM was written"


def test_builder_equals_engine(engine, builder):
    """The builder object on the same heights gives the engine's map and mask."""
    torch = _gpu()
    z = torch.from_numpy(crater()).cuda()
    torch.cuda.synchronize()
    hz = {"max_slope_deg": 15.0, "inflate": 7.0, "min_cells": 2}
    a, ma = engine.build_costmap(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, hazard=hz, return_mask=True)
    b, mb = builder.build(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, dem=(z.data_ptr(), N, N, -HW, -HW, RES),
                          hazard=hz, return_mask=True)
    assert np.array_equal(a, b) and np.array_equal(ma, mb)
    assert builder.last_ms() > 0
    out = torch.zeros((SIZE, SIZE), dtype=torch.float32, device="cuda")
    assert builder.build(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, out_device=out.data_ptr(),
                         dem=(z.data_ptr(), N, N, -HW, -HW, RES), hazard=hz) is None
    assert np.array_equal(out.cpu().numpy(), a)


def test_borrowed_device_dem():
    """mppi_build_costmap_hazard reads a DEM borrowed by set_dem_device in place."""
    torch = _gpu()
    from mppi_amd import _lib
    z = torch.from_numpy(crater()).cuda()
    torch.cuda.synchronize()
    eng = _lib.Engine(_lib.make_params(256, 20), 0)
    try:
        eng.set_dem_device(z.data_ptr(), N, N, HW, keepalive=z)
        got, mask = eng.build_costmap(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, hazard=scene.Hazard(15.0, 7.0),
                                      return_mask=True)
        H0, H1 = crater_occupancy(15.0, 1, 7.0)
        d = discs("rocks40")
        check("borrowed", got, mask, HR.expected_map(H1 | d, POWER, "chamfer"), HR.expected_mask(H0, H1, d))
        # the terrain changes in place: the caller rebuilds, and the new map follows the new heights
        z.zero_()
        torch.cuda.synchronize()
        eng.dem_updated()
        got, mask = eng.build_costmap(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, hazard=scene.Hazard(15.0, 7.0),
                                      return_mask=True)
        assert not (mask & 3).any()
        assert np.array_equal(got, HR.expected_map(d, POWER, "chamfer"))
    finally:
        eng.close()


# ---- 3. hz == NULL / hazard=None: the existing entry points, bitwise ----
def test_off_means_untouched(engine, builder):
    _gpu()
    lib = engine.lib
    from mppi_amd import _lib
    obs, optr = _lib._obstacles(ROCKS["rocks40"])
    for metric in METRICS:
        m = _lib.COSTMAP_METRICS[metric]
        want = CR.create_obstacles_costmap(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER) if metric == "exact" else \
            CR.create_obstacles_costmap_cv(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER)
        old = engine.build_costmap(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, metric=metric)
        assert np.array_equal(old, want)
        assert np.array_equal(engine.build_costmap(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, metric=metric,
                                                   hazard=None), old)
        out = np.empty((SIZE, SIZE), np.float32)
        mask = np.full((SIZE, SIZE), 0xAB, np.uint8)
        rc = lib.mppi_build_costmap_hazard(engine.ctx, optr, len(obs), SIZE, HW, ORIGIN[0], ORIGIN[1], RR, POWER, None,
                                           _lib._fp(out), mask.ctypes.data_as(C.POINTER(C.c_uint8)), m)
        assert rc == 0 and np.array_equal(out, old) and (mask == 0xAB).all()
        out2 = np.empty((SIZE, SIZE), np.float32)
        rc = lib.mppi_costmap_builder_build_hazard(builder.h, optr, len(obs), SIZE, HW, ORIGIN[0], ORIGIN[1], RR, POWER,
                                                   None, 0, 0, 0.0, 0.0, 0.0, None, _lib._fp(out2), None, None, m)
        assert rc == 0 and np.array_equal(out2, old)
        assert np.array_equal(builder.build(ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, metric=metric), old)


# ---- 4. the batch: a crater field and its hazard map never leave the device ----
KB, HB, STEPS = 64, 20, 6
STARTS = ((-60.0, -5.0), (10.0, 12.0))


def _batch_run(fill):
    from mppi_amd import _lib
    eng = _lib.Engine(_lib.make_params(KB, HB), 0)
    try:
        eng.set_dem(np.zeros((N, N), np.float32), HW)
        eng.set_costmap(np.zeros((SIZE, SIZE), np.float32), HW)
        batch = _lib.Batch(eng, 2)
        extra = fill(batch)
        for e in range(2):
            batch.set_episode(e, V.mppi_state(B.start_state(STARTS[e], V.FAR)), 100 + e, dem=3, costmap=5)
        batch.run(STEPS, "3d", _lib.make_policy(**B.RUN))
        out = []
        for e in range(2):
            res = V.collect(batch, e)
            res["rows"] = batch.log(e)
            res["steps"] = len(res["rows"])
            out.append(res)
        batch.close()
    finally:
        eng.close()
    return out, extra


def test_batch_slot_from_crater_field():
    _gpu()
    hz = scene.Hazard(15.0, 7.0)
    field = scene.CraterField(scene.BUMPS_9)

    def on_device(batch):
        Z = batch.build_dem(3, field, HW, copy_out=True)
        cm, mask = batch.build_costmap_hazard(5, ROCKS["rocks40"], ORIGIN, RR, hz, 3, POWER, copy_out=True,
                                              return_mask=True)
        return Z, cm, mask

    got, (Z, cm, mask) = _batch_run(on_device)
    want, want_mask = HR.expected_build(Z, -HW, -HW, RES, ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, "chamfer", 15.0,
                                        1, hz.inflate)
    check("batch slot", cm, mask, want, want_mask)
    assert (mask & 1).any() and not np.array_equal(cm, HR.expected_map(discs("rocks40"), POWER, "chamfer"))

    def uploaded(batch):
        batch.set_dem(3, Z)
        batch.set_costmap(5, cm)

    twin, _ = _batch_run(uploaded)
    for e in range(2):
        assert got[e]["steps"] == STEPS
        V.same(got[e], twin[e], f"episode {e}")


def test_batch_context_dem_and_no_mask():
    """dem = -1 reads the context's DEM; without copy_out and return_mask nothing is downloaded."""
    _gpu()
    from mppi_amd import _lib
    eng = _lib.Engine(_lib.make_params(KB, HB), 0)
    try:
        eng.set_dem(crater(), HW)
        eng.set_costmap(np.zeros((SIZE, SIZE), np.float32), HW)
        batch = _lib.Batch(eng, 1)
        assert batch.build_costmap_hazard(0, [], ORIGIN, RR, {"max_slope_deg": 20.0, "inflate": 0.0}) is None
        cm, mask = batch.build_costmap_hazard(1, [], ORIGIN, RR, {"max_slope_deg": 20.0, "inflate": 0.0}, metric="exact",
                                              copy_out=True, return_mask=True)
        plain = batch.build_costmap(2, [[1.0, 2.0, 3.0]], ORIGIN, RR, POWER, copy_out=True)
        assert np.array_equal(batch.build_costmap_hazard(3, [[1.0, 2.0, 3.0]], ORIGIN, RR, None, copy_out=True), plain)
        H0, H1 = crater_occupancy(20.0, 1, 0.0)
        none = np.zeros_like(H0)
        check("context dem", cm, mask, HR.expected_map(H1, POWER, "exact"), HR.expected_mask(H0, H1, none))
        batch.close()
    finally:
        eng.close()


# ---- 5. refusals ----
def test_refusals(builder):
    torch = _gpu()
    from mppi_amd import _lib
    lib = builder.lib
    inf, nan = float("inf"), float("nan")
    z = torch.from_numpy(crater()).cuda()
    torch.cuda.synchronize()

    def refused(rc, word, code=MPPI_EINVAL):
        assert rc == code, (rc, lib.mppi_last_error())
        assert word.encode() in lib.mppi_last_error(), (word, lib.mppi_last_error())

    bad = [((0.0, 1.0, 1, 0), "max_slope_deg"), ((90.0, 1.0, 1, 0), "max_slope_deg"), ((-3.0, 1.0, 1, 0), "max_slope_deg"),
           ((nan, 1.0, 1, 0), "max_slope_deg"), ((inf, 1.0, 1, 0), "max_slope_deg"), ((15.0, -1.0, 1, 0), "inflate"),
           ((15.0, nan, 1, 0), "inflate"), ((15.0, inf, 1, 0), "inflate"), ((15.0, 3.0e9, 1, 0), "int32"),
           ((15.0, 1.0, 0, 0), "min_cells"), ((15.0, 1.0, -2, 0), "min_cells"), ((15.0, 1.0, 1, 7), "reserved")]
    eng = _lib.Engine(_lib.make_params(KB, HB), 0)
    try:
        ctx_call = lambda hz: lib.mppi_build_costmap_hazard(eng.ctx, None, 0, SIZE, HW, 0.0, 0.0, RR, POWER,   # noqa: E731
                                                            C.byref(hz), None, None, 0)
        refused(ctx_call(_lib.MppiHazard(15.0, 1.0, 1, 0)), "no DEM", MPPI_ESTATE)
        eng.set_dem(crater(), HW)
        eng.set_costmap(np.zeros((SIZE, SIZE), np.float32), HW)
        batch = _lib.Batch(eng, 1)
        slot_call = lambda hz, dem=-1: lib.mppi_batch_build_costmap_hazard(batch.h, 0, dem, None, 0, 0.0, 0.0, RR,   # noqa: E731
                                                                          POWER, 0, C.byref(hz), None, None)
        bld_call = lambda hz, ptr=z.data_ptr(): lib.mppi_costmap_builder_build_hazard(   # noqa: E731
            builder.h, None, 0, SIZE, HW, 0.0, 0.0, RR, POWER, C.c_void_p(ptr), N, N, -HW, -HW, RES, C.byref(hz), None,
            None, None, 0)
        for fields, word in bad:
            for call in (ctx_call, slot_call, bld_call):
                refused(call(_lib.MppiHazard(*fields)), word)
        ok = _lib.MppiHazard(15.0, 1.0, 1, 0)
        refused(slot_call(ok, 9), "dem_slot 9", MPPI_ESTATE)          # an empty DEM slot
        refused(slot_call(ok, 256), "256")                            # outside the table
        refused(bld_call(ok, None), "no DEM", MPPI_ESTATE)
        refused(lib.mppi_build_costmap_hazard(None, None, 0, SIZE, HW, 0.0, 0.0, RR, POWER, C.byref(ok), None, None, 0),
                "null")
        # the refusals left everything usable
        assert ctx_call(ok) == 0 and slot_call(ok) == 0 and bld_call(ok) == 0
        batch.close()
    finally:
        eng.close()
    with pytest.raises(ValueError):
        builder.build([], ORIGIN, SIZE, HW, RR, hazard=scene.Hazard(15.0))         # no dem=
    with pytest.raises(ValueError):
        builder.build([], ORIGIN, SIZE, HW, RR, return_mask=True)                   # a mask needs a hazard


# ---- 6. the controller: Surface.hazard, rebuild_costmap, costmaps= entries ----
def _controller(k=KB):
    from mppi_amd import controller
    cfg = controller._load_config(controller.DEFAULT_CONFIG)
    cfg = {**cfg, "controller": {**cfg["controller"], "number_of_trajectories": k, "number_of_iterations": HB},
           "engine": {**(cfg.get("engine") or {}), "seed": 11}}
    surface = controller.Surface.from_arrays(crater(), np.zeros((SIZE, SIZE), np.float32), HW, radius_robot=RR)
    robot = controller.Robot(STARTS[0][0], STARTS[0][1], [1.0, 0.0, 0.0], cfg)
    ctl = controller.MPPI_Controller(surface, robot, cfg, V.FAR[0], V.FAR[1], 0.0)
    ctl.std_dev_u1 = ctl.std_dev_u2 = 0.25
    return ctl


def test_controller_rebuild_and_campaign_entries():
    _gpu()
    from mppi_amd import controller
    assert controller.Surface.hazard is None
    hz = scene.Hazard(15.0)                                   # inflate None: r_robot + 0.1
    d = discs("rocks40")
    H0, H1 = crater_occupancy(15.0, 1, float(np.float32(RR + 0.1)))
    ctl = _controller()
    ctl.warp_setup()
    try:
        plain = ctl.rebuild_costmap(ROCKS["rocks40"], ORIGIN)
        assert np.array_equal(plain, HR.expected_map(d, POWER, "chamfer"))
        assert np.array_equal(ctl.rebuild_costmap(ROCKS["rocks40"], ORIGIN, hazard=hz),
                              HR.expected_map(H1 | d, POWER, "chamfer"))
        ctl.surface.hazard = hz
        assert np.array_equal(ctl.rebuild_costmap(ROCKS["rocks40"], ORIGIN), HR.expected_map(H1 | d, POWER, "chamfer"))
        assert np.array_equal(ctl.rebuild_costmap(ROCKS["rocks40"], ORIGIN, hazard=None), plain)
        ctl.surface.hazard = None
    finally:
        ctl.engine.close()
    # one crater field per task with its matching hazard map, against the same maps given as arrays
    from mppi_amd import _lib
    field = scene.CraterField(scene.BUMPS_9)
    db = _lib.DemBuilder(0)
    built = db.build(field, N, HW)            # the heights the DEM slot holds, as the device builds them
    db.close()
    infl = float(np.float32(RR + 0.1))
    with_slot, _ = HR.expected_build(built, -HW, -HW, RES, ROCKS["rocks40"], ORIGIN, SIZE, HW, RR, POWER, "chamfer",
                                     15.0, 1, infl)
    _, H1c = crater_occupancy(20.0, 1, infl)
    entry = {"obstacles": ROCKS["rocks40"], "origin": ORIGIN}
    on_device = [{**entry, "hazard": hz, "dem": 0}, {**entry, "hazard": {"max_slope_deg": 20.0}}, entry]
    as_arrays = [with_slot, HR.expected_map(H1c | d, POWER, "chamfer"), plain]
    assert not np.array_equal(with_slot, plain) and not np.array_equal(as_arrays[1], plain)
    res = []
    for dems, costmaps in (([field], on_device), ([built], as_arrays)):
        ctl = _controller()
        try:
            res.append(ctl.run_campaign([STARTS[0]] * 3, [(1.0, 0.0, 0.0)] * 3, [V.FAR] * 3, seeds=[5, 6, 7], lanes=2,
                                        max_loops=[4, 4, 4], dems=dems, costmaps=costmaps, task_dem=[0, -1, -1],
                                        task_costmap=[0, 1, 2]))
        finally:
            ctl.engine.close()
    for i, (a, w) in enumerate(zip(*res)):
        assert a["loops"] == w["loops"] == 4
        for key in ("x", "y", "z", "lin_vel", "ang_vel"):
            assert np.array_equal(np.asarray(a[key], np.float32).view(np.uint32),
                                  np.asarray(w[key], np.float32).view(np.uint32)), (i, key)
