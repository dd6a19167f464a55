#!/usr/bin/env python3
"""C3 steps at a raised temperature (default T = 3000: every 32-trajectory line of every leaf holds a
non-zero softmax weight, so leaf_records takes its dense layout), timed as bench.py times the
headline: back-to-back steps with the deferred tail, `--reps` runs of `--steps` steps.

Usage: python profiles/leaf_dense_timing.py [--temperature 3000] [--steps 200] [--warmup 20] [--reps 5]
MPPI_LIB_PATH selects another build of the library (A/B against the parent).  Prints one JSON line:
us per step of every run, their median and spread, and the server's own rollout / step clocks.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--temperature", type=float, default=3000.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-K", type=int, default=65536)
    ap.add_argument("-H", type=int, default=100)
    args = ap.parse_args()
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()
    eng = _lib.Engine(_lib.make_params(args.K, args.H, temperature=args.temperature), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    eng.set_state(_lib.make_state(-60.0, -5.0, (1.0, 0.0, 0.0), goal_x=65.0, goal_y=10.0))
    eng.set_async_tail(True)
    runs = []
    step = 0
    try:
        for _ in range(args.warmup):
            eng.step("3d", step, copy=False)
            step += 1
        for _ in range(args.reps):
            eng.outputs()
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.step("3d", step, copy=False)
                step += 1
            eng.outputs()
            eng.sync()
            runs.append((time.perf_counter() - t0) / args.steps * 1e6)
        r_us, s_us, n = eng.server_time()
        info = eng.launch_info()
    finally:
        eng.close()
    runs_sorted = sorted(runs)
    print(json.dumps(dict(temperature=args.temperature, K=args.K, H=args.H, steps=args.steps,
                          us_per_step=[round(x, 2) for x in runs],
                          median_us=round(runs_sorted[len(runs) // 2], 2),
                          spread_us=round(runs_sorted[-1] - runs_sorted[0], 2),
                          server_rollout_us=round(r_us / n, 2) if n else None,
                          server_step_us=round(s_us / n, 2) if n else None,
                          resident=info["resident"], server_launches=info["server_launches"],
                          lib=os.environ.get("MPPI_LIB_PATH") or "default")))


if __name__ == "__main__":
    main()
