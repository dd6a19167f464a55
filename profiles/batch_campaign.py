#!/usr/bin/env python3
"""A campaign on a batch's task queue (mppi_batch_set_tasks / _run_tasks) against the
same tasks run as plain batches, at the reference's configuration K = 1 000, H = 100, E = 64.

Workload: N = 512 far-goal tasks whose lengths are their step caps, a fixed list between 50 and 400
steps (task_caps below), so every count is exact and reproducible.

  campaign  set_tasks, run_tasks until every task has ended, task / task_log of all N, score_tasks
  plain8    the same tasks as 8 plain batches of 64 in list order, as a user runs them without the
            queue: set_episode x 64, run to the batch's longest cap, episode / log x 64, score
  step      per-step wall time of one plain batch of 64 that calls no task entry point (`--steps`)
  common    a campaign of 64 tasks with one common cap: the campaign form of the finish, no refill
  refill    a campaign of 64 x `--steps` tasks of cap 1: every lane refills in every step

Median of `--repeats` repeats after a warm-up; wall time by perf_counter, with the HIP-event time
(mppi_batch_get_ms) beside it.  `--legs plain8 step` uses the entry points of the plain batch only, so
the same file measures an older build; `--pkg` names the directory that holds the mppi_amd package to
import (default this tree's), and `--parent FILE...` embeds such runs' outputs.  Prints one JSON line
and writes profiles/batch/campaign.json unless --out / --no-write.

    timeout 600 python profiles/batch_campaign.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, GOAL = (-60.0, -5.0), (65.0, 10.0)
LEGS = ("campaign", "plain8", "step", "common", "refill")


def task_caps(n=512):
    """The fixed list of step caps, 50 .. 399: a sawtooth that falls by 2 or 3 steps per task and wraps
    every 134 tasks or so, so a plain batch of 64 consecutive tasks spans about 170 steps."""
    return [50 + (i * 2654435761 >> 7) % 351 for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--tasks", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd"))
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    for p in (ROOT, a.pkg):
        sys.path.insert(0, p)

    import torch
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()
    E, N = a.lanes, a.tasks
    caps = task_caps(N)

    def start(i):
        return _lib.make_state(START[0] + 0.05 * (i % 16), START[1] - 0.05 * ((i // 16) % 32), goal_x=GOAL[0],
                               goal_y=GOAL[1])

    eng = _lib.Engine(_lib.make_params(a.K, a.H, seed=42), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    batch = _lib.Batch(eng, E)

    def median_of(fn):
        runs = [fn() for _ in range(a.repeats + 1)][1:]          # the first run is the warm-up
        out = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        out["wall_s_min"] = min(r["wall_s"] for r in runs)
        out["wall_s_max"] = max(r["wall_s"] for r in runs)
        return {k: round(v, 6) for k, v in out.items()}

    def campaign(tasks, readback):
        t0 = time.perf_counter()
        batch.set_tasks(tasks)
        done, steps, ms = 0, 0, 0.0
        while done < len(tasks):
            done, s = batch.run_tasks(1 << 20)
            steps += s
            ms += batch.last_ms()
        t1 = time.perf_counter()
        rows = 0
        if readback:
            for i in range(len(tasks)):
                rows += len(batch.task_log(i, 0, batch.task(i)["steps"]))
            batch.score_tasks()
        t2 = time.perf_counter()
        return dict(wall_s=t2 - t0, run_wall_s=t1 - t0, event_ms=ms, batch_steps=steps, rows=rows)

    def plain8():
        t0 = time.perf_counter()
        steps, ms, rows, run_wall = 0, 0.0, 0, 0.0
        for b0 in range(0, N, E):
            part = list(range(b0, min(b0 + E, N)))
            for e, i in enumerate(part):
                batch.set_episode(e, start(i), 1000 + i)
            n = max(caps[i] for i in part)
            t1 = time.perf_counter()
            batch.run(n)
            run_wall += time.perf_counter() - t1
            steps += n
            ms += batch.last_ms()
            for e, i in enumerate(part):                  # the task's own rows: up to its cap
                rows += len(batch.log(e, 0, min(caps[i], batch.episode(e)["steps_last_run"])))
            batch.score()
        return dict(wall_s=time.perf_counter() - t0, run_wall_s=run_wall, event_ms=ms, batch_steps=steps, rows=rows)

    def step():
        for e in range(E):
            batch.set_episode(e, start(e), 42 + e)
        t0 = time.perf_counter()
        batch.run(a.steps)
        wall = time.perf_counter() - t0
        return dict(wall_s=wall, event_ms=batch.last_ms(), us_per_step=1e6 * wall / a.steps)

    def timed_campaign(tasks, steps_expected):
        batch.set_tasks(tasks)
        t0 = time.perf_counter()
        done, steps = batch.run_tasks(1 << 20)
        wall = time.perf_counter() - t0
        assert done == len(tasks) and steps == steps_expected, (done, steps)
        return dict(wall_s=wall, event_ms=batch.last_ms(), us_per_step=1e6 * wall / steps)

    res = dict(K=a.K, H=a.H, lanes=E, tasks=N, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               caps_min=min(caps), caps_max=max(caps), caps_sum=sum(caps), caps=caps)
    if "campaign" in a.legs:
        from mppi_amd.batch import campaign_makespan
        tasks = [_lib.make_task(start(i), 1000 + i, caps[i]) for i in range(N)]
        res["campaign"] = median_of(lambda: campaign(tasks, True))
        res["campaign_makespan"] = campaign_makespan(caps, E)
        assert res["campaign"]["batch_steps"] == res["campaign_makespan"], res["campaign"]
        assert res["campaign"]["rows"] == sum(caps)
    if "plain8" in a.legs:
        res["plain8"] = median_of(plain8)
    if "step" in a.legs:
        res["step"] = median_of(step)
    if "common" in a.legs:
        tasks = [_lib.make_task(start(i), 42 + i, a.steps) for i in range(E)]
        res["common"] = median_of(lambda: timed_campaign(tasks, a.steps))
    if "refill" in a.legs:
        tasks = [_lib.make_task(start(i), 42 + i, 1) for i in range(E * a.steps)]
        res["refill"] = median_of(lambda: timed_campaign(tasks, a.steps))
    batch.close()
    eng.close()
    if "campaign" in res and "plain8" in res:
        res["wall_ratio_plain8_over_campaign"] = round(res["plain8"]["wall_s"] / res["campaign"]["wall_s"], 3)
        res["step_ratio_plain8_over_campaign"] = round(res["plain8"]["batch_steps"] / res["campaign"]["batch_steps"], 3)
    if a.parent:
        res["parent"] = [json.load(open(p)) for p in a.parent]
        for p in res["parent"]:
            p.pop("caps", None)
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        out = a.out or os.path.join(ROOT, "profiles", "batch", "campaign.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
