#!/usr/bin/env python3
"""Throughput of a batch whose episodes hold parameter variants, at the shape of
profiles/batch_throughput.py (K = 1 000, H = 100, E = 64, 200 steps, far goal).

Three legs on one engine, each the median of `--repeats` repeats after a warm-up run:
  plain     no variant entry point is called (what batch_throughput.py --only 64 measures)
  variants  the 64 episodes spread over 8 variants, four 2D and four 3D (weights, temperature and
            filters varied), so every step launches the rollout kernel once per projection and
            half of each launch's workgroups return at once
  score     Batch.score() of the 64 executed paths of the last run: the kernel's HIP-event time
            (mppi_get_score_ms) and the wall time of the call
Prints one JSON line; --write stores it as profiles/batch/variants_throughput.json.

    timeout 600 python profiles/batch_variants.py
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
    ap.add_argument("--legs", nargs="*", default=["plain", "variants"])
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()

    import torch
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()
    eng = _lib.Engine(_lib.make_params(a.K, a.H, seed=42), 0)
    eng.set_dem(Z, hw)
    eng.set_costmap(cm, hw)

    def seed_state(e):
        return _lib.make_state(START[0] + 0.05 * (e % 16), START[1] - 0.05 * (e // 16), goal_x=GOAL[0], goal_y=GOAL[1])

    table = []
    for i in range(8):
        table.append(_lib.make_variant("2d" if i % 2 == 0 else "3d", w_slope=50.5 - 5.0 * i, w_obstacle=25.0 + 10.0 * i,
                                       temperature=0.3 * (1 + i), filter_a=0.96 - 0.01 * i, opt_filter_k=3.0 - 0.1 * i))

    res = dict(K=a.K, H=a.H, E=a.E, steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    for leg in a.legs:
        batch = _lib.Batch(eng, a.E)
        if leg == "variants":
            batch.set_variants(table)
        walls, mss = [], []
        for rep in range(a.repeats + 1):          # the first run is the warm-up
            for e in range(a.E):
                if leg == "variants":
                    batch.set_episode(e, seed_state(e), 42 + e, e % 8)
                else:                             # the variant entry points are not touched
                    _lib._check(eng.lib, eng.lib.mppi_batch_set_episode(batch.h, e, seed_state(e), 42 + e), "set_episode")
            t0 = time.perf_counter()
            batch.run(a.steps)
            walls.append(time.perf_counter() - t0)
            mss.append(batch.last_ms())
        ran = [batch.episode(e)["steps_last_run"] for e in range(a.E)]
        assert min(ran) == a.steps, f"an episode stopped early: {min(ran)} steps"
        wall, ms = statistics.median(walls[1:]), statistics.median(mss[1:])
        res[leg] = dict(wall_s=round(wall, 6), wall_s_min=round(min(walls[1:]), 6), wall_s_max=round(max(walls[1:]), 6),
                        event_ms=round(ms, 3), episode_steps_per_s=round(a.E * a.steps / wall, 1),
                        us_per_step=round(1e6 * wall / a.steps, 2))
        if leg == a.legs[-1]:
            sw, sk = [], []
            for rep in range(a.repeats + 1):
                t0 = time.perf_counter()
                sc = batch.score()
                sw.append(time.perf_counter() - t0)
                sk.append(eng.score_ms())
            assert int(sc["rows"].min()) == a.steps
            res["score"] = dict(paths=a.E, rows=a.steps, kernel_ms=round(statistics.median(sk[1:]), 4),
                                wall_ms=round(1e3 * statistics.median(sw[1:]), 4), bytes_out=24 * a.E)
        batch.close()
    eng.close()
    if "plain" in res and "variants" in res:
        res["variants_over_plain_wall"] = round(res["variants"]["wall_s"] / res["plain"]["wall_s"], 4)
    line = json.dumps(res)
    print(line)
    if a.write:
        out = os.path.join(ROOT, "profiles", "batch")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "variants_throughput.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
