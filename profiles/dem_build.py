#!/usr/bin/env python3
"""Build times of the on-device crater-field DEM builder (mppi_dem_builder_*) at the
thesis's terrain: 1500^2 cells, half-width 75 m.

  nine      the 9-crater list (scene.BUMPS_9), both variants: HIP-event time of the factor and product
            kernels (mppi_dem_builder_last_ms) and the wall time of Engine.build_dem (upload of the
            crater rows, the kernels, the normal table, the verified reciprocal; no copy out)
  field     4 500 craters drawn uniformly (RandomState(5): cx, cy ~ U(-75, 75), height ~ U(0.6, 4.5),
            width ~ U(0.5, 3.0)), one per 5 m^2: the same two figures
  normals   the normal table alone (Engine.dem_updated, wall)
  host      the path this replaces: scene.crater_dem on the host for the 9-crater list, and
            Engine.set_dem of the result (upload + normal table).  The host time of the 4 500-crater
            field is EXTRAPOLATED from it (x 500: the loop's cost is per crater), not run.

Median, minimum and maximum of `--repeats` runs after one warm-up.  Prints one JSON line.

    timeout 600 python profiles/dem_build.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID, HW = 1500, 75.0


def stats(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--field", type=int, default=4500)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd"))
    a = ap.parse_args()
    for p in (ROOT, a.pkg):
        sys.path.insert(0, p)

    import numpy as np
    import torch
    from mppi_amd import _lib, scene

    rng = np.random.RandomState(5)
    field = np.stack([rng.uniform(-HW, HW, a.field), rng.uniform(-HW, HW, a.field), rng.uniform(0.6, 4.5, a.field),
                      rng.uniform(0.5, 3.0, a.field)], 1)
    lists = {"nine": scene.crater_rows(scene.BUMPS_9), "field": field}
    out = dict(device=torch.cuda.get_device_name(0), grid=GRID, half_width=HW, repeats=a.repeats,
               craters={k: int(v.shape[0]) for k, v in lists.items()})

    b = _lib.DemBuilder(0)
    eng = _lib.Engine(_lib.make_params(256, 20), 0)
    dev = torch.empty((GRID, GRID), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for name, rows in lists.items():
        for variant in ("mfma", "valu"):
            ev, wall = [], []
            for r in range(a.repeats + 1):
                b.build(rows, GRID, HW, out_device=dev.data_ptr(), variant=variant)
                t0 = time.perf_counter()
                eng.build_dem(rows, GRID, HW, copy_out=False, variant=variant)
                t1 = time.perf_counter()
                if r:
                    ev.append(b.last_ms())
                    wall.append((t1 - t0) * 1e3)
            out[f"{name}_{variant}_kernels_ms"] = stats(ev)
            out[f"{name}_{variant}_engine_build_wall_ms"] = stats(wall)
    wall = []
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        eng.dem_updated()
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    out["normal_table_wall_ms"] = stats(wall)

    host, upload = [], []
    for r in range(a.host_repeats):
        t0 = time.perf_counter()
        Z = scene.crater_dem(GRID, HW, scene.BUMPS_9)
        t1 = time.perf_counter()
        eng.set_dem(Z, HW)
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3)
        upload.append((t2 - t1) * 1e3)
    out["host_nine_crater_dem_ms"] = stats(host)
    out["host_nine_set_dem_ms"] = stats(upload)
    out["host_field_crater_dem_ms_extrapolated"] = round(statistics.median(host) * a.field / 9.0, 1)
    got = b.build(lists["nine"], GRID, HW)
    out["nine_cells_differing_from_host"] = int(np.count_nonzero(got != Z))
    b.close()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
