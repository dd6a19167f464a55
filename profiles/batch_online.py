#!/usr/bin/env python3
"""A campaign scored while it runs (mppi_batch_set_tasks_scored) against the same
campaign logged and scored afterwards, at the configuration of profiles/batch_campaign.py: K = 1 000,
H = 100, 64 lanes, the 512 far-goal tasks of task_caps (50 .. 399 steps, 118 216 in all).

  logged     set_tasks, run_tasks to the end, then score_tasks: the log arena and the second pass
  scored     set_tasks(scored=True): the same arena, the scores come from the lanes (task_scores)
  log_free   set_tasks(scored=True, keep_log=False): no arena

Per leg: the batch steps per second of the run (wall clock around run_tasks, which ends in a stream
wait, and the HIP-event time beside it), the time of what follows the run (score_tasks, or
task_scores), and the device memory per task: the bytes the tables and the arena need by their
layouts, and the drop of free device memory over set_tasks on a fresh batch.  The three legs
alternate within every repeat; the first repeat is the warm-up and is dropped; the medians and the
run-to-run spread of `--repeats` repeats are reported.  The three legs' scores are compared bitwise.
Prints one JSON line and writes profiles/batch/online.json unless --out / --no-write.

    timeout 600 python profiles/batch_online.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_campaign import GOAL, START, task_caps  # noqa: E402

LEGS = ("logged", "scored", "log_free")
TASK_BYTES, RESULT_BYTES, SCORE_BYTES, ROW_BYTES = 88, 56, 40, 32      # csrc/mppi_kernels.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--tasks", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
        sys.path.insert(0, p)

    import numpy as np
    import torch
    from mppi_amd import _lib, scene
    from mppi_amd.batch import campaign_makespan

    if not torch.cuda.is_available():
        raise SystemExit("batch_online.py measures on the GPU: no HIP device")
    Z, hw, cm = scene.scene_c3()
    E, N = a.lanes, a.tasks
    caps = task_caps(N)
    makespan = campaign_makespan(caps, E)

    def start(i):
        return _lib.make_state(START[0] + 0.05 * (i % 16), START[1] - 0.05 * ((i // 16) % 32), goal_x=GOAL[0],
                               goal_y=GOAL[1])

    eng = _lib.Engine(_lib.make_params(a.K, a.H, seed=42), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    tasks = [_lib.make_task(start(i), 1000 + i, caps[i]) for i in range(N)]
    set_args = dict(logged={}, scored=dict(scored=True), log_free=dict(scored=True, keep_log=False))

    # device memory: free memory over set_tasks on a fresh batch (the allocator's granularity shows)
    mem = {}
    for leg in LEGS:
        b = _lib.Batch(eng, E)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        b.set_tasks(tasks, **set_args[leg])
        mem[leg] = free0 - torch.cuda.mem_get_info(0)[0]
        b.close()
    batch = _lib.Batch(eng, E)

    def run(leg):
        t0 = time.perf_counter()
        batch.set_tasks(tasks, **set_args[leg])
        t1 = time.perf_counter()
        done, steps, ms = 0, 0, 0.0
        while done < N:
            done, s = batch.run_tasks(1 << 20)
            steps += s
            ms += batch.last_ms()
        t2 = time.perf_counter()
        scores = batch.score_tasks() if leg == "logged" else batch.task_scores()
        t3 = time.perf_counter()
        assert steps == makespan, (leg, steps, makespan)
        return dict(set_s=t1 - t0, run_wall_s=t2 - t1, event_ms=ms, score_s=t3 - t2, wall_s=t3 - t0,
                    steps_per_s=steps / (t2 - t1)), scores

    runs = {leg: [] for leg in LEGS}
    scores = {}
    for rep in range(a.repeats + 1):
        for leg in LEGS:
            r, scores[leg] = run(leg)
            if rep > 0:          # the first repeat is the warm-up
                runs[leg].append(r)
    for leg in ("scored", "log_free"):
        for k in ("cost", "terms", "collisions", "rows"):
            assert np.array_equal(np.asarray(scores[leg][k]).view(np.uint32),
                                  np.asarray(scores["logged"][k]).view(np.uint32)), (leg, k)
    assert np.array_equal(scores["scored"]["length"], scores["log_free"]["length"])
    batch.close()
    eng.close()

    res = dict(K=a.K, H=a.H, lanes=E, tasks=N, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               caps_sum=sum(caps), batch_steps=makespan)
    per_task = dict(logged=TASK_BYTES + RESULT_BYTES, scored=TASK_BYTES + RESULT_BYTES + SCORE_BYTES,
                    log_free=TASK_BYTES + RESULT_BYTES + SCORE_BYTES)
    for leg in LEGS:
        rs = runs[leg]
        out = {k: statistics.median(r[k] for r in rs) for k in rs[0]}
        out["run_wall_s_min"] = min(r["run_wall_s"] for r in rs)
        out["run_wall_s_max"] = max(r["run_wall_s"] for r in rs)
        out["us_per_step"] = 1e6 * out["run_wall_s"] / makespan
        arena = 0 if leg == "log_free" else ROW_BYTES * (sum(caps) + max(caps))
        out["bytes_per_task"] = per_task[leg] + arena / N
        out["free_memory_drop_bytes"] = mem[leg]
        res[leg] = {k: round(v, 6) if isinstance(v, float) else v for k, v in out.items()}
    a_, c_ = res["logged"], res["log_free"]
    res["logged_spread_us_per_step"] = round(1e6 * (a_["run_wall_s_max"] - a_["run_wall_s_min"]) / makespan, 4)
    res["log_free_minus_logged_us_per_step"] = round(c_["us_per_step"] - a_["us_per_step"], 4)
    res["scored_minus_logged_us_per_step"] = round(res["scored"]["us_per_step"] - a_["us_per_step"], 4)
    res["scores_bitwise_equal"] = True
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        out = a.out or os.path.join(ROOT, "profiles", "batch", "online.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
