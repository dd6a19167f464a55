#!/usr/bin/env python3
"""Time of the path-scoring kernel at the headline config C3 (K = 65 536, H = 100).

One sampled step, then Engine.cost_terms(): the step is re-run with device-side dump buffers and
mppi_score_kernel reads them, 40 bytes per waypoint (traj, lw, rw: 12 each, v: 4).  Prints one JSON
line: the kernel's HIP-event time, its input bytes, the implied GB/s and fraction of the 8 TB/s HBM
peak, and beside it the HIP-event time of a device-to-device copy of the same number of bytes measured
in the same process (independent of the scoring code; it reads and writes, so it moves twice the traffic).

    timeout 300 python profiles/score_paths.py [--reps 7] > profiles/score_paths.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=65536)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()

    import numpy as np
    import torch
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()
    eng = _lib.Engine(_lib.make_params(a.K, a.H), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    eng.set_state(_lib.make_state(-60.0, -5.0, goal_x=65.0, goal_y=10.0))
    eng.step("3d", 0)
    costs = eng.costs()
    score = []
    for _ in range(a.reps + 1):          # the first call is the warm-up
        terms, col = eng.cost_terms()
        score.append(eng.score_ms())
    score = score[1:]
    p = eng.params
    re = np.float32(p.w_path) * terms[:, 0]
    for w, k in ((p.w_slope, 1), (p.w_speed, 2), (p.w_obstacle, 3)):
        re = re + np.float32(w) * terms[:, k]
    eng.close()

    nbytes = 40 * a.K * a.H
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.zero_()
    copy = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copy.append(e0.elapsed_time(e1))
    copy = copy[1:]

    ms = statistics.median(score)
    cms = statistics.median(copy)
    print(json.dumps(dict(
        config="C3", K=a.K, H=a.H, device=torch.cuda.get_device_name(0), reps=a.reps,
        score_ms=round(ms, 4), score_ms_min=round(min(score), 4), score_ms_max=round(max(score), 4),
        input_bytes=nbytes, score_GBps=round(nbytes / ms / 1e6, 1),
        fraction_of_8TBps=round(nbytes / ms / 1e6 / 8000.0, 4),
        d2d_copy_ms=round(cms, 4), d2d_copy_ms_min=round(min(copy), 4),
        d2d_copy_GBps_read_plus_write=round(2 * nbytes / cms / 1e6, 1),
        score_over_copy=round(ms / cms, 3),
        recombined_equals_costs=bool(np.array_equal(re.astype(np.float32), costs)),
        collisions_total=int(col.sum()))))


if __name__ == "__main__":
    main()
