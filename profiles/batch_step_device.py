#!/usr/bin/env python3
"""The batch's device-resident step (mppi_batch_step_device) against the two ways a
plant outside the controller could reach the batch before it, at K = 1 000, H = 100, E = 64.

Three legs, alternated `--rounds` times in one process after a warm-up of each:

  run     mppi_batch_run, `--steps` steps in one call: the plant is the controller's own model and the
          state feedback is the finish kernel's advance lane.  The floor: nothing crosses to the host.
  device  Batch.step_device `--steps` times with a trivial plant on the device (a torch unicycle
          integrated from cmd, the Isaac loop's sigmas from w) on the engine's stream, which is a
          torch stream bound with set_stream.  No host synchronisation inside the timed region, one
          at its end.  Two figures: with the plant, and with the states left as they are (the step
          alone: ingest, noise, rollout, finish).
  host    the host-fed route: per step E set_episode calls (each zeroes the warm start and waits for
          the stream), run(1) and E episode() readbacks, `--host-steps` steps.

  tracked (--tracked) the device leg with tracking set (mppi_batch_set_tracking): four more figures, the
          step alone with keep_log on / off and z given / NULL (the DEM lookup), every run long enough
          that no episode ends inside the timed region; the untracked step alone is timed beside them
          in the same rounds.  Written to profiles/batch/step_tracked.json.

Per-step wall time by perf_counter around work that ends in a stream synchronise.  `launch` is the
time of one empty-ish kernel launch in the same job (a one-element torch add, enqueued 2 000 times,
then one synchronise): what one more launch per step costs when launches are back to back.
Prints one JSON line and writes profiles/batch/step_device.json unless --out / --no-write.

    timeout 600 python profiles/batch_step_device.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, GOAL = (-60.0, -5.0), (65.0, 10.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tracked", action="store_true", help="time the tracked device step instead of the three legs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
        sys.path.insert(0, p)

    import numpy as np
    import torch
    from mppi_amd import _lib, scene
    from mppi_amd.batch import ISAAC_POLICY, pack_states, state_dict

    if not torch.cuda.is_available():
        raise SystemExit("batch_step_device.py needs a GPU: no figure is reported without one")
    E, H, n = a.episodes, a.H, a.steps
    Z, hw, cm = scene.scene_c3()
    eng = _lib.Engine(_lib.make_params(a.K, H), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    pol = _lib.make_policy(**ISAAC_POLICY)
    # E rovers on a line left of the map, all driving to the far goal
    starts = [state_dict(START[0], START[1] + 0.5 * (e - E / 2), (1.0, 0.0, 0.0), 0.0, 0.0, GOAL[0], GOAL[1])
              for e in range(E)]
    first = pack_states(starts)
    mstates = [_lib.make_state(s["x"], s["y"], s["heading"], 0.0, 0.0, s["goal_x"], s["goal_y"]) for s in starts]

    def fill(batch):
        for e in range(E):
            batch.set_episode(e, mstates[e], 100 + e)

    dt, radius = float(eng.params.dt), float(eng.params.robot_radius)

    def plant(states, cmd):
        v, w = cmd[:, 0], cmd[:, 1]
        hx, hy = states[:, 2].clone(), states[:, 3].clone()
        c, s = torch.cos(w * dt), torch.sin(w * dt)
        states[:, 0] += v * hx * dt
        states[:, 1] += v * hy * dt
        states[:, 2] = c * hx - s * hy
        states[:, 3] = s * hx + c * hy
        states[:, 5] = v - w * radius / 2
        states[:, 6] = v + w * radius / 2
        ww = w * w / 3.0
        states[:, 9] = torch.clamp(0.25 - ww, min=0.25)
        states[:, 10] = torch.clamp(0.25 + ww, min=0.25)

    batch = _lib.Batch(eng, E)
    with torch.cuda.stream(stream):
        states = torch.as_tensor(first).cuda()
        cmd = torch.zeros((E, 2), dtype=torch.float32, device="cuda")
        plan = torch.zeros((E, 4 * H + 12), dtype=torch.float32, device="cuda")
        one = torch.zeros(1, device="cuda")
        zpose = torch.full((E,), 0.25, dtype=torch.float32, device="cuda")
        done = torch.zeros(E, dtype=torch.int32, device="cuda")
    stream.synchronize()

    def stat(v):
        return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2),
                    all=[round(x, 2) for x in v])

    def emit(res, name):
        line = json.dumps(res)
        print(line)
        if not a.no_write:
            out = a.out or os.path.join(ROOT, "profiles", "batch", name)
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "w") as f:
                f.write(line + "\n")

    def leg_run():
        fill(batch)
        t0 = time.perf_counter()
        batch.run(n, "3d", pol)
        t = time.perf_counter() - t0
        steps = batch.episode(0)["steps_last_run"]
        return t / steps * 1e6, batch.last_ms() / steps * 1e3

    def leg_device(with_plant):
        fill(batch)
        with torch.cuda.stream(stream):
            states.copy_(torch.as_tensor(first), non_blocking=False)
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                batch.step_device(states, cmd=cmd, plan=plan)
                if with_plant:
                    plant(states, cmd)
            stream.synchronize()
            t = time.perf_counter() - t0
        assert batch.episode(0)["steps_total"] == n
        return t / n * 1e6

    def leg_tracked(keep_log, with_z):
        fill(batch)
        batch.set_tracking(max_steps=n + 1, keep_log=keep_log, goal_tol=0.5)
        with torch.cuda.stream(stream):
            states.copy_(torch.as_tensor(first), non_blocking=False)
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                batch.step_device(states, cmd=cmd, plan=plan, z=zpose if with_z else None, done=done)
            stream.synchronize()
            t = time.perf_counter() - t0
        assert batch.episode(0)["steps_total"] == n and not done.any().item()
        batch.clear_tracking()
        return t / n * 1e6

    def leg_host():
        fill(batch)
        cur = list(mstates)
        t0 = time.perf_counter()
        for _ in range(a.host_steps):
            for e in range(E):
                batch.set_episode(e, cur[e], 100 + e)
            batch.run(1, "3d", pol)
            cur = [batch.episode(e)["state"] for e in range(E)]
        return (time.perf_counter() - t0) / a.host_steps * 1e6

    def leg_launch(m=2000):
        with torch.cuda.stream(stream):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(m):
                one.add_(1.0)
            stream.synchronize()
            return (time.perf_counter() - t0) / m * 1e6

    if a.tracked:
        forms = dict(log_z=(True, True), log_dem=(True, False), nolog_z=(False, True), nolog_dem=(False, False))
        leg_device(False)
        for kw in forms.values():
            leg_tracked(*kw)
        rows = dict(device_alone=[], **{k: [] for k in forms})
        for _ in range(a.rounds):
            rows["device_alone"].append(leg_device(False))
            for k, kw in forms.items():
                rows[k].append(leg_tracked(*kw))
        batch.close()
        eng.close()
        med = {k: statistics.median(v) for k, v in rows.items()}
        res = dict(what="batch_step_tracked", K=a.K, H=H, E=E, steps=n, rounds=a.rounds, unit="us per batch step",
                   **{k: stat(v) for k, v in rows.items()})
        res["tracked_minus_device_alone_us"] = {k: round(med[k] - med["device_alone"], 2) for k in forms}
        res["device_alone_spread_us"] = round(max(rows["device_alone"]) - min(rows["device_alone"]), 2)
        emit(res, "step_tracked.json")
        return

    # warm-up: every leg once at its timed shape (code objects loaded, the log grown, torch's kernels built)
    leg_run(), leg_device(True), leg_device(False), leg_host(), leg_launch()
    rows = dict(run_wall=[], run_event=[], device_plant=[], device_alone=[], host=[], launch=[])
    for _ in range(a.rounds):
        w, ev = leg_run()
        rows["run_wall"].append(w)
        rows["run_event"].append(ev)
        rows["device_plant"].append(leg_device(True))
        rows["device_alone"].append(leg_device(False))
        rows["host"].append(leg_host())
        rows["launch"].append(leg_launch())
    batch.close()
    eng.close()

    res = dict(what="batch_step_device", K=a.K, H=H, E=E, steps=n, host_steps=a.host_steps, rounds=a.rounds,
               unit="us per batch step", **{k: stat(v) for k, v in rows.items()})
    med = {k: statistics.median(v) for k, v in rows.items()}
    res["device_alone_minus_run_us"] = round(med["device_alone"] - med["run_wall"], 2)
    res["device_plant_minus_run_us"] = round(med["device_plant"] - med["run_wall"], 2)
    res["run_spread_us"] = round(max(rows["run_wall"]) - min(rows["run_wall"]), 2)
    res["episode_steps_per_s"] = {k: round(E / med[k] * 1e6) for k in ("run_wall", "device_plant", "device_alone",
                                                                         "host")}
    emit(res, "step_device.json")


if __name__ == "__main__":
    main()
