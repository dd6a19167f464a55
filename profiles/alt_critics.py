#!/usr/bin/env python3
"""The cost of the critic set (mppi_set_critics): three measurements.

  default   the headline `ms_per_step` of bench.py (C3, the other legs switched off) of a parent build
            (`--parent DIR`: a checkout of the parent commit with its library built) and of this
            tree, alternating, `--runs` fresh processes each.  The new median must lie inside the
            parent's own min-max spread of this job.
  modes     C3 (K = 65 536, H = 100): the rollout kernel's HIP-event time under mppi_set_timing(2),
            separate launches, 3D and 2D, each for {wheels, body, body + orientation}; `--repeats`
            passes of `--steps` steps each, the passes' averages reported as median / min / max.
  batch     64 episodes, K = 1 000, H = 100, 200 steps, half under a 2D body variant and half under a
            3D wheels variant (the thesis's 2D-vs-3D slope comparison as one batch), at the shape of
            profiles/batch_variants.py's "64 episodes over 8 variants" row.

Prints one JSON line and writes profiles/alt_critics.json unless --no-write.

    timeout 900 python profiles/alt_critics.py --parent ../parent
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, GOAL = (-60.0, -5.0), (65.0, 10.0)
BENCH = ["--gpus", "1", "--steps", "200", "--warmup", "20", "--no-c4", "--no-c5", "--no-shard", "--no-costmap",
         "--no-cadence", "--no-bilinear", "--no-sync-pass", "--cpu-baseline-seconds", "0"]
SETS = (("wheels", dict(slope="wheels", w_orientation=0.0)), ("body", dict(slope="body", w_orientation=0.0)),
        ("body+orientation", dict(slope="body", w_orientation=1000.0)))


def headline(tree):
    """ms_per_step of one bench.py process run in `tree`."""
    out = subprocess.run([sys.executable, "bench.py"] + BENCH, cwd=tree, check=True, capture_output=True, text=True,
                         timeout=300).stdout
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    return rec["ms_per_step"]


def spread(xs, digits=5):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits),
                runs=[round(x, digits) for x in xs])


def leg_default(a):
    parent, new = [], []
    for _ in range(a.runs):
        parent.append(headline(a.parent))
        new.append(headline(ROOT))
    r = dict(parent=spread(parent), new=spread(new))
    r["new_median_inside_parent_spread"] = bool(min(parent) <= statistics.median(new) <= max(parent))
    r["new_median_not_slower_than_parent_max"] = bool(statistics.median(new) <= max(parent))
    return r


def leg_modes(a, _lib, scene):
    Z, hw, cm = scene.scene_c3()
    K, H = 65536, 100
    eng = _lib.Engine(_lib.make_params(K, H, seed=42), 0)
    eng.set_option("resident", 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    eng.set_state(_lib.make_state(START[0], START[1], goal_x=GOAL[0], goal_y=GOAL[1]))
    res = {}
    for proj in ("3d", "2d"):
        for name, crit in SETS:
            eng.set_critics(**crit)
            eng.set_timing(False)
            for i in range(20):
                eng.step(proj, i, copy=False)
            avgs = []
            for rep in range(a.repeats):
                eng.set_timing(2)
                r0, _, n0 = eng.timing()
                for i in range(a.steps):
                    eng.step(proj, 20 + rep * a.steps + i, copy=False)
                eng.sync()
                r1, _, n1 = eng.timing()
                avgs.append(1e3 * (r1 - r0) / max(n1 - n0, 1))
                eng.set_timing(False)
            r = dict(rollout_us=spread(avgs, 2), block=eng.launch_info().get("block"))
            if proj == "3d":
                # where the time goes (mppi_get_chain_clock, one reading per step; the 2D chain takes no
                # stamps): workgroup 0's chain wave, from its end to the last role's, its leaf, and the
                # span from the first workgroup's start to the last one's record
                clk = []
                for i in range(20):
                    eng.step(proj, 5000 + i, copy=False)
                    clk.append(eng.chain_clock())
                for key, field, digits in (("chain_cycles_per_step", "cycles_per_step", 1), ("chain_us", "chain_us", 2),
                                           ("start_to_chain_us", "start_to_chain_us", 2),
                                           ("chain_end_to_roles_done_us", "chain_to_roles_done_us", 2),
                                           ("leaf_us", "leaf_us", 2), ("wg_start_spread_us", "wg_start_spread_us", 2),
                                           ("wg_span_us", "wg_span_us", 2)):
                    r[key] = round(statistics.median(c[field] for c in clk), digits)
            res[f"{proj} {name}"] = r
    eng.close()
    return res


def leg_batch(a, _lib, scene):
    from mppi_amd.batch import variant_dict
    Z, hw, cm = scene.scene_c3()
    K, H, E, steps = 1000, 100, 64, 200
    eng = _lib.Engine(_lib.make_params(K, H, seed=42), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)
    batch = _lib.Batch(eng, E)
    batch.set_variants([dict(variant_dict("2d"), slope="body"), dict(variant_dict("3d"), slope="wheels")])
    walls, mss = [], []
    for rep in range(a.repeats + 1):          # the first run is the warm-up
        for e in range(E):
            st = _lib.make_state(START[0] + 0.05 * (e % 16), START[1] - 0.05 * (e // 16), goal_x=GOAL[0], goal_y=GOAL[1])
            batch.set_episode(e, st, 42 + e, e % 2)
        t0 = time.perf_counter()
        batch.run(steps)
        walls.append(time.perf_counter() - t0)
        mss.append(batch.last_ms())
    ran = [batch.episode(e)["steps_last_run"] for e in range(E)]
    assert min(ran) == steps, f"an episode stopped early: {min(ran)} steps"
    batch.close()
    eng.close()
    wall = statistics.median(walls[1:])
    return dict(K=K, H=H, E=E, steps=steps, us_per_step=round(1e6 * wall / steps, 2),
                us_per_step_min=round(1e6 * min(walls[1:]) / steps, 2), us_per_step_max=round(1e6 * max(walls[1:]) / steps, 2),
                event_ms=round(statistics.median(mss[1:]), 3), episode_steps_per_s=round(E * steps / wall, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="*", default=["default", "modes", "batch"])
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
        sys.path.insert(0, p)
    res = {}
    if "default" in a.legs:
        if not a.parent:
            sys.exit("the default leg needs --parent DIR")
        res["default"] = leg_default(a)     # (before this process opens the GPU: one process at a time)
    if "modes" in a.legs or "batch" in a.legs:
        import torch
        from mppi_amd import _lib, scene
        res["device"] = torch.cuda.get_device_name(0)
        if "modes" in a.legs:
            res["modes"] = leg_modes(a, _lib, scene)
        if "batch" in a.legs:
            res["batch"] = leg_batch(a, _lib, scene)
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "alt_critics.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
