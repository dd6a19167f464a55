#!/usr/bin/env python3
"""Closed-loop throughput of the batched episodes (mppi_batch_*) against one Engine
stepped from the host, at the reference's own configuration K = 1 000, H = 100.

Baseline: one Engine at its default options running the closed loop from the host (set_state, step,
read row 0 and v / w, the advance rule on the host), `--steps` steps with a far goal so that nothing
terminates.  Batches of E = 1, 16, 64, 256 episodes run the same number of steps with one
mppi_batch_run call.  Median of `--repeats` repeats after a warm-up run; episode-steps per second by
wall time, with the HIP-event time of the run (mppi_batch_get_ms) beside it.  Prints one JSON line
and writes profiles/batch/throughput.json.

    timeout 600 python profiles/batch_throughput.py
    # one batch size only, nothing written (e.g. under rocprofv3 --kernel-trace --stats):
    python profiles/batch_throughput.py --only 64 --repeats 1 --no-write
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


def host_loop(eng, steps, seed_state, radius):
    """run()'s loop on one Engine with the least host work a Python caller can do: the state struct
    is updated in place from the engine's output buffers (no copies, Python float arithmetic: a
    timing loop, its trail agrees with the float32 rule of the batch to the last few bits only)."""
    from mppi_amd import batch
    st = seed_state()
    buf = eng._buf
    t0 = time.perf_counter()
    for i in range(steps):
        eng.set_state(st)
        eng.step("3d", i, copy=False)
        traj, hv = buf["traj_sim"], buf["heading_sim"]
        v, w = float(buf["lin_vel"][0]), float(buf["ang_vel"][0])
        h = batch.normalise_heading(hv[:3])
        st.x, st.y = float(traj[0]), float(traj[1])
        st.heading[0], st.heading[1], st.heading[2] = float(h[0]), float(h[1]), float(h[2])
        ww = w * w
        st.std_dev_u1, st.std_dev_u2 = max(0.4, 0.4 - ww), max(0.4, 0.4 + ww)
        half = w * radius / 2
        st.left_wheel_speed, st.right_wheel_speed = v - half, v + half
    return time.perf_counter() - t0, (st.x, st.y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16, 64, 256])
    ap.add_argument("--only", type=int, default=None, help="one batch size, no baseline")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()

    import torch
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()

    def seed_state(e=0):
        # (episodes differ in start pose and seed, as a campaign's do)
        return _lib.make_state(START[0] + 0.05 * (e % 16), START[1] - 0.05 * (e // 16), goal_x=GOAL[0], goal_y=GOAL[1])

    def engine(seed=42):
        eng = _lib.Engine(_lib.make_params(a.K, a.H, seed=seed), 0)
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        return eng

    res = dict(K=a.K, H=a.H, steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    if a.only is None:
        walls = []
        for rep in range(a.repeats + 1):          # the first run is the warm-up
            eng = engine()
            wall, end = host_loop(eng, a.steps, seed_state, float(eng.params.robot_radius))
            info = eng.launch_info()
            eng.close()
            walls.append(wall)
        wall = statistics.median(walls[1:])
        res["baseline"] = dict(wall_s=round(wall, 6), wall_s_min=round(min(walls[1:]), 6),
                               episode_steps_per_s=round(a.steps / wall, 1), us_per_step=round(1e6 * wall / a.steps, 2),
                               server_steps=info["server_steps"], end_xy=[round(end[0], 4), round(end[1], 4)])
    res["batch"] = {}
    eng = engine()
    for E in ([a.only] if a.only is not None else a.batches):
        batch = _lib.Batch(eng, E)
        walls, mss = [], []
        for rep in range(a.repeats + 1):
            for e in range(E):
                batch.set_episode(e, seed_state(e), 42 + e)
            t0 = time.perf_counter()
            batch.run(a.steps)
            walls.append(time.perf_counter() - t0)
            mss.append(batch.last_ms())
        ran = [batch.episode(e)["steps_last_run"] for e in range(E)]
        assert min(ran) == a.steps, f"an episode stopped early: {min(ran)} steps"
        s = batch.episode(0)["state"]
        batch.close()
        wall, ms = statistics.median(walls[1:]), statistics.median(mss[1:])
        res["batch"][str(E)] = dict(wall_s=round(wall, 6), wall_s_min=round(min(walls[1:]), 6), event_ms=round(ms, 3),
                                    episode_steps_per_s=round(E * a.steps / wall, 1),
                                    us_per_step=round(1e6 * wall / a.steps, 2), end_xy_episode0=[round(s.x, 4), round(s.y, 4)])
        if "baseline" in res:
            res["batch"][str(E)]["speedup_vs_baseline"] = round(
                res["batch"][str(E)]["episode_steps_per_s"] / res["baseline"]["episode_steps_per_s"], 2)
    eng.close()
    if "baseline" in res and "64" in res["batch"]:
        res["ratio_E64"] = res["batch"]["64"]["speedup_vs_baseline"]
        res["target_ratio_E64"] = 16.0
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        out = os.path.join(ROOT, "profiles", "batch")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "throughput.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
