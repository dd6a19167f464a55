#!/usr/bin/env python3
"""Sampling plans against the number of trajectories: one scored campaign on the C3 scene
(MPPI_Controller.run_campaign with score=True, log=False).

  tasks        `--tasks` start/goal pairs 30 to 45 m apart around the map, each with its own seed
  K            1000, 500, 350 (task_trajectories)
  plans        default, nominal, antithetic, nominal + antithetic, and the same four with beta = 0.7
  projections  2D and 3D

Every (K, plan, projection) group runs the same tasks with the same seeds; the table is
mppi_amd.batch.campaign_summary keyed by the group.  Prints the table as Markdown and writes it with
the raw groups as JSON (`--out`, default profiles/sampling_campaign.json).  No threshold: the table is
recorded whichever way it falls.

    timeout 900 python profiles/sampling_campaign.py
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
    sys.path.insert(0, p)

KS = (1000, 500, 350)
BASE_PLANS = (("default", {}), ("nominal", dict(nominal=True)), ("antithetic", dict(antithetic=True)),
              ("nominal+antithetic", dict(nominal=True, antithetic=True)))
PLANS = BASE_PLANS + tuple((n + ", beta 0.7", dict(p, noise_beta=0.7)) for n, p in BASE_PLANS)
PROJS = ("2d", "3d")


def tasks(n):
    """n (start, heading, goal): starts on a ring of radius 45 m about the map's centre, the goal 30 to
    45 m further along a chord, the heading towards it."""
    out = []
    for i in range(n):
        a = 2.0 * math.pi * i / n
        sx, sy = 45.0 * math.cos(a), 45.0 * math.sin(a)
        b = a + math.pi * (0.55 + 0.25 * ((i * 7) % 5) / 4.0)
        d = 30.0 + 15.0 * ((i * 3) % 7) / 6.0
        gx, gy = sx + d * math.cos(b), sy + d * math.sin(b)
        out.append(((sx, sy), (math.cos(b), math.sin(b), 0.0), (gx, gy)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=24)
    ap.add_argument("--max-loops", type=int, default=900)
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_campaign.json"))
    a = ap.parse_args()

    import numpy as np
    from mppi_amd import controller, scene
    from mppi_amd.batch import campaign_results, campaign_summary, variant_dict

    Z, hw, cm = scene.scene_c3()
    cfg = controller._load_config(controller.DEFAULT_CONFIG)
    cfg = {**cfg, "controller": {**cfg["controller"], "number_of_trajectories": max(KS), "number_of_iterations": a.H}}
    surface = controller.Surface.from_arrays(Z, cm, hw)
    robot = controller.Robot(0.0, 0.0, [1.0, 0.0, 0.0], cfg)
    ctl = controller.MPPI_Controller(surface, robot, cfg, 0.0, 0.0, 0.0)

    base = tasks(a.tasks)
    variants, names = [], []
    for proj in PROJS:
        for name, keys in PLANS:
            variants.append(dict(variant_dict(proj), **keys))
            names.append((name, proj))
    starts, headings, goals, seeds, tv, tk, by = [], [], [], [], [], [], []
    for K in KS:
        for v, (name, proj) in enumerate(names):
            for i, (s, h, g) in enumerate(base):
                starts.append(s)
                headings.append(h)
                goals.append(g)
                seeds.append(1000 + i)
                tv.append(v)
                tk.append(K)
                by.append(f"K={K} | {proj} | {name}")
    t0 = time.perf_counter()
    res, scores = ctl.run_campaign(starts, headings, goals, seeds=seeds, lanes=a.lanes, max_loops=a.max_loops,
                                   variants=variants, task_variant=tv, task_trajectories=tk, score=True, log=False)
    wall = time.perf_counter() - t0
    ctl.engine.close()
    table = campaign_summary(campaign_results(res, scores), by)
    loops = {}
    for r, k in zip(res, by):
        loops.setdefault(k, []).append(r["loops"])
    lines = ["| K | proj | plan | reached | collided | mean cost | mean obstacle | mean length [m] | mean loops |",
             "|---|---|---|---|---|---|---|---|---|"]
    for k, row in table.items():
        K, proj, name = [s.strip() for s in k.split("|")]
        m = row["mean"]
        lines.append(f"| {K[2:]} | {proj} | {name} | {row['reached']}/{row['count']} | {row['collided']} | "
                     f"{m['cost']:.4g} | {m['obstacle']:.4g} | {m['length']:.2f} | {np.mean(loops[k]):.0f} |")
    print("\n".join(lines))
    print(f"{len(starts)} tasks on {a.lanes} lanes, cap {a.max_loops} steps, H = {a.H}: {wall:.1f} s")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tasks=a.tasks, max_loops=a.max_loops, lanes=a.lanes, H=a.H, wall_s=round(wall, 2),
                       table=table, mean_loops={k: float(np.mean(v)) for k, v in loops.items()},
                       markdown=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
