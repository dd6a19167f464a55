#!/usr/bin/env python3
"""The cost of the wheel log, the wheel form of the online slope chain and the online path metrics
(mppi_batch_set_wheel_log / _set_score_options) per batch step, at the configuration of
profiles/batch_throughput.py: K = 1 000, H = 100, E = 64 far-goal episodes, `--steps` steps.

Three ways a closed loop runs on the device, each with the options off and on:

  run       mppi_batch_run:                         off | wheel log
  campaign  a scored list that keeps no log:        off | wheel slope chain | metrics | both
  tracked   mppi_batch_step_tracked, keep_log = 0:  off | wheel slope chain | metrics | both
            (keep_log = 1: off | wheel log)

`campaign`: 64 lanes, 64 tasks with the cap `--steps`, so every lane runs one task to its cap and the run
is `--steps` batch steps.  `tracked`: the plant is a fixed table of poses on the device (no model in the
loop), one enqueue per step and one wait at the end.  The legs of a group alternate within every repeat;
the first repeat is the warm-up and is dropped; medians of the HIP-event time (run, campaign) or the wall
time (tracked) per step over `--repeats` repeats, with the spread (max - min) of the `off` leg beside
them.  Prints one JSON line and writes profiles/batch/wheels.json unless --no-write.

    timeout 600 python profiles/batch_wheels.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

START, GOAL = (-60.0, -5.0), (65.0, 10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()
    E, n = a.E, a.steps

    def state(e):
        return _lib.make_state(START[0] + 0.05 * (e % 16), START[1] - 0.05 * (e // 16), goal_x=GOAL[0], goal_y=GOAL[1])

    eng = _lib.Engine(_lib.make_params(a.K, a.H, seed=42), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)

    def run_leg(wheel_log):
        batch = _lib.Batch(eng, E)
        if wheel_log:
            batch.set_wheel_log()
        for e in range(E):
            batch.set_episode(e, state(e), 42 + e)
        batch.run(n)
        ms = batch.last_ms()
        assert min(batch.episode(e)["steps_last_run"] for e in range(E)) == n
        batch.close()
        return 1e3 * ms / n

    def campaign_leg(slope, metrics):
        batch = _lib.Batch(eng, E)
        tasks = [_lib.make_task(state(e), 42 + e, n) for e in range(E)]
        batch.set_tasks(tasks, scored=dict(slope=slope, metrics=metrics) if (slope != "body" or metrics) else True,
                        keep_log=False)
        done, ms = 0, 0.0
        while done < E:
            done, _ = batch.run_tasks(n)
            ms += batch.last_ms()
        batch.close()
        return 1e3 * ms / n

    # the tracked plant: poses that drift along x, written once; a step reads table[i]
    table = np.zeros((n + 1, E, 11), np.float32)
    for e in range(E):
        s = state(e)
        for i in range(n + 1):
            table[i, e] = (s.x + 0.09 * i, s.y + 0.01 * i, 1.0, 0.0, 0.0, 0.5, 0.5, GOAL[0], GOAL[1], 0.4, 0.4)
    dev = torch.as_tensor(table).cuda()

    def tracked_leg(slope, metrics, keep_log=False, wheel_log=False):
        batch = _lib.Batch(eng, E)
        if wheel_log:
            batch.set_wheel_log()
        for e in range(E):
            batch.set_episode(e, state(e), 42 + e)
        batch.set_tracking(max_steps=n + 1, keep_log=keep_log, slope=slope, metrics=metrics)
        cmd = torch.empty((E, 2), dtype=torch.float32, device="cuda")
        plan = torch.empty((E, 4 * a.H + 12), dtype=torch.float32, device="cuda")
        done = torch.empty((E,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n + 1):
            batch.step_device(dev[i], cmd=cmd, plan=plan, done=done)
        eng.sync()
        wall = time.perf_counter() - t0
        batch.close()
        return 1e6 * wall / (n + 1)

    groups = {
        "run": {"off": lambda: run_leg(False), "wheel_log": lambda: run_leg(True)},
        "campaign_log_free": {"off": lambda: campaign_leg("body", False), "wheel_chain": lambda: campaign_leg("wheels", False),
                              "metrics": lambda: campaign_leg("body", True), "both": lambda: campaign_leg("wheels", True)},
        "tracked_log_free": {"off": lambda: tracked_leg("body", False), "wheel_chain": lambda: tracked_leg("wheels", False),
                             "metrics": lambda: tracked_leg("body", True), "both": lambda: tracked_leg("wheels", True)},
        "tracked_logged": {"off": lambda: tracked_leg("body", False, True), "wheel_log": lambda: tracked_leg("body", False, True, True)},
    }
    res = dict(K=a.K, H=a.H, E=E, steps=n, repeats=a.repeats, device=torch.cuda.get_device_name(0), unit="us per batch step")
    for g, legs in groups.items():
        seen = {k: [] for k in legs}
        for rep in range(a.repeats + 1):
            for k, f in legs.items():
                seen[k].append(f())
        res[g] = {k: round(statistics.median(v[1:]), 3) for k, v in seen.items()}
        res[g]["off_spread"] = round(max(seen["off"][1:]) - min(seen["off"][1:]), 3)
    eng.close()
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        out = os.path.join(ROOT, "profiles", "batch")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "wheels.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
