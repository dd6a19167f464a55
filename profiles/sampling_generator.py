#!/usr/bin/env python3
"""The normals generator under each sampling plan, as the workload of a kernel trace.

Runs `--steps` separate-launch steps at C3 (K = 65 536, H = 100, "resident" 0, so the generator is a
kernel of its own in the trace) and `--steps` steps of a 64-episode batch (K = 1 000, H = 100) under one
plan.  The time per kernel is read from the trace's statistics, a run of its own per plan:

    rocprofv3 --kernel-trace --stats -d OUT -o k --output-format csv -- \
        python profiles/sampling_generator.py --plan antithetic

(mppi_noise_kernel / mppi_noise_plan_kernel / mppi_noise_serial_kernel, and mppi_batch_noise_kernel /
mppi_batch_noise_plan_kernel).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
    sys.path.insert(0, p)

PLANS = {"default": {}, "antithetic": dict(antithetic=True), "nominal": dict(nominal=True),
         "beta": dict(beta=0.7), "combined": dict(antithetic=True, nominal=True, beta=0.7)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default="default", choices=sorted(PLANS))
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()
    state = _lib.make_state(-60.0, -5.0, (1.0, 0.0, 0.0), goal_x=65.0, goal_y=10.0)
    eng = _lib.Engine(_lib.make_params(65536, 100), 0)
    eng.set_option("resident", 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    eng.set_state(state)
    eng.set_sampling(**PLANS[a.plan])
    for i in range(a.steps):
        eng.step("3d", i, copy=False)
    eng.outputs()
    eng.close()

    eng = _lib.Engine(_lib.make_params(1000, 100), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    eng.set_sampling(**PLANS[a.plan])
    batch = _lib.Batch(eng, 64)
    for e in range(64):
        batch.set_episode(e, state, 42 + e)
    batch.run(a.steps)
    batch.close()
    eng.close()
    print(f"plan {a.plan}: {a.steps} C3 steps and {a.steps} batch steps done")


if __name__ == "__main__":
    main()
