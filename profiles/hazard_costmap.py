#!/usr/bin/env python3
"""Build times of the hazard costmap (mppi_costmap_builder_build_hazard) at the
thesis's scene (1500^2 DEM over +-75 m, 750^2 costmap) and at the 8192^2 DEM / 1024^2 costmap scene
(+-102.4 m), both with the 9-crater field built on the device, 750 rocks, a 15 degree limit and the
reference's margin r_robot + 0.1 as the inflation.

  rock_only   the build without a hazard (mppi_costmap_builder_last_ms, HIP events)
  hazard      the build with it (the same events: count, H0, the exact passes, H1, then as before);
              both with the default chamfer metric
  hazard_exact  the build with it and the exact metric: the map the host route below computes
  count       the steep-cell count kernel alone (mppi_costmap_builder_hazard_count_ms)
  copy        a device-to-device copy of Z (torch, HIP events), alternated with the builds in the same
              run: the count kernel's yardstick.  It reads what the copy reads and writes almost
              nothing, so count / copy above 1 means the pass is not streaming.  bytes/s are the
              DEM's bytes (rows * cols * 4) over each time.
  host_route  the path this replaces, wall clock: heights to the host, scene.hazard_occupancy, the
              rock raster and scene.edt_costmap on the host, Engine.set_costmap (upload).  Its map is
              the exact-metric one (scipy's EDT; no chamfer exists on the host without OpenCV) and
              is compared with the device's exact-metric map.  --host-repeats 0 skips it.

Each event figure is one operation between two events, so at the small scene it contains the event
pair's own overhead (a few microseconds), the same for the kernel and for the copy.  The mask of
every timed scene is compared with scene.hazard_occupancy on the downloaded heights first.
Median, minimum and maximum of `--repeats` runs after a warm-up.  Prints one JSON line.

    timeout 900 python profiles/hazard_costmap.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"c3_1500_750": (1500, 75.0, 750), "c5_8192_1024": (8192, 102.4, 1024)}
R_ROBOT, POWER, DEG = 1.2, 20, 15.0


def stats(xs):
    return dict(median=round(statistics.median(xs), 5), min=round(min(xs), 5), max=round(max(xs), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--pkg", default=os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd"))
    a = ap.parse_args()
    for p in (ROOT, a.pkg):
        sys.path.insert(0, p)

    import numpy as np
    import torch
    from mppi_amd import _lib, scene

    if not torch.cuda.is_available():
        raise SystemExit("hazard_costmap.py measures on the GPU: none is visible")
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, max_slope_deg=DEG, inflate=R_ROBOT + 0.1)
    rocks = scene.random_obstacles()
    hz = scene.Hazard(DEG)
    cb, db = _lib.CostmapBuilder(0), _lib.DemBuilder(0)
    for name in a.scenes.split(","):
        grid, hw, size = SCENES[name]
        res = 2.0 * hw / grid
        z = torch.empty((grid, grid), dtype=torch.float32, device="cuda")
        z2 = torch.empty_like(z)
        cm = torch.empty((size, size), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        db.build(scene.BUMPS_9, grid, hw, out_device=z.data_ptr())
        dem = (z.data_ptr(), grid, grid, -hw, -hw, res)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        rock, haz, hex_, cnt, cpy = [], [], [], [], []
        for r in range(a.repeats + 3):
            cb.build(rocks, (0.0, 0.0), size, hw, R_ROBOT, POWER, out_device=cm.data_ptr())
            t_rock = cb.last_ms()
            cb.build(rocks, (0.0, 0.0), size, hw, R_ROBOT, POWER, out_device=cm.data_ptr(), dem=dem, hazard=hz)
            t_haz, t_cnt = cb.last_ms(), cb.hazard_count_ms()
            cb.build(rocks, (0.0, 0.0), size, hw, R_ROBOT, POWER, out_device=cm.data_ptr(), dem=dem, hazard=hz,
                     metric="exact")
            t_hex = cb.last_ms()
            ev[0].record()
            z2.copy_(z)
            ev[1].record()
            torch.cuda.synchronize()
            if r >= 3:
                rock.append(t_rock)
                haz.append(t_haz)
                hex_.append(t_hex)
                cnt.append(t_cnt)
                cpy.append(ev[0].elapsed_time(ev[1]))
        s = dict(dem=grid, costmap=size, rock_only_ms=stats(rock), hazard_ms=stats(haz), hazard_exact_ms=stats(hex_), count_ms=stats(cnt),
                 copy_ms=stats(cpy))
        zbytes = grid * grid * 4
        s["count_over_copy"] = round(s["count_ms"]["median"] / s["copy_ms"]["median"], 3)
        s["count_read_GBps"] = round(zbytes / s["count_ms"]["median"] / 1e6, 1)
        s["copy_read_GBps"] = round(zbytes / s["copy_ms"]["median"] / 1e6, 1)
        # the same result as the numpy statement, at the size that was timed
        got, mask = cb.build(rocks, (0.0, 0.0), size, hw, R_ROBOT, POWER, dem=dem, hazard=hz, return_mask=True,
                             metric="exact")
        if a.host_repeats < 1:
            out[name] = s
            del z, z2, cm
            continue
        eng = _lib.Engine(_lib.make_params(256, 20), 0)
        eng.set_costmap(np.zeros((size, size), np.float32), hw)
        host = []
        for r in range(a.host_repeats):
            t0 = time.perf_counter()
            Zh = z.cpu().numpy()
            H0, H1 = scene.hazard_occupancy(Zh, -hw, -hw, res, size, hw, DEG, 1, R_ROBOT + 0.1)
            x = np.linspace(-hw, hw, size)
            X, Y = np.meshgrid(x, x)
            occ = H1.copy()
            for xg, yg, rr in rocks:
                tr = rr / 2 + R_ROBOT + 0.1
                occ |= (X - yg) ** 2 + (Y - xg) ** 2 <= tr ** 2
            host_map = scene.edt_costmap(occ, POWER)
            eng.set_costmap(host_map, hw)
            host.append((time.perf_counter() - t0) * 1e3)
        eng.close()
        s["host_route_wall_ms"] = stats(host)
        s["mask_equals_numpy"] = bool(np.array_equal(mask & 1, H0) and np.array_equal(mask >> 1 & 1, H1))
        s["exact_map_equals_host"] = bool(np.array_equal(got, host_map))
        s["h0_cells"], s["h1_cells"] = int(H0.sum()), int(H1.sum())
        out[name] = s
        del z, z2, cm
    cb.close()
    db.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
