#!/usr/bin/env python3
"""Throughput of a batch whose episodes hold their own DEM, costmap and trajectory count
(DESIGN.md §3.7), at the shape of profiles/batch_throughput.py (K = 1 000, H = 100, E = 64, 200
steps, far goal, the C3 scene).

Legs, each the median of `--repeats` repeats after a warm-up run:
  plain     no scene or variant entry point is called (what batch_variants.py's plain leg measures:
            run it on the parent commit's build too, alternating, for the null-pointer rule)
  slots1    the 64 episodes on one DEM slot and one costmap slot holding copies of the context's
            scene: the cost of the indirection alone
  slots8    the episodes spread over 8 DEM slots and 8 costmap slots (the heights scaled and the
            costmap shifted per slot)
  dems64    one DEM slot per episode, each 1500^2 heights and a 36 MB normal table (about 2.9 GB):
            what 64 different normal tables cost in L2 / MALL
  mixedk    the episodes split over K_e = 1000 / 500 / 350 in one batch, against the sum of three
            batches of the same episode counts on contexts of those K
  score     Batch.score() with every path on its own episode's costmap (8 slots), and without
Prints one JSON line; --write stores it as profiles/batch/scenes_throughput.json.

    timeout 900 python profiles/batch_scenes.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "husky-rover-mppi-isaacsim_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

START, GOAL = (-60.0, -5.0), (65.0, 10.0)
LEGS = ["plain", "slots1", "slots8", "dems64", "mixedk", "score"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", nargs="*", default=LEGS)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()

    import torch
    from mppi_amd import _lib, scene

    Z, hw, cm = scene.scene_c3()

    def engine(K):
        eng = _lib.Engine(_lib.make_params(K, a.H, seed=42), 0)
        eng.set_dem(Z, hw)
        eng.set_costmap(cm, hw)
        return eng

    def seed_state(e):
        return _lib.make_state(START[0] + 0.05 * (e % 16), START[1] - 0.05 * (e // 16), goal_x=GOAL[0], goal_y=GOAL[1])

    def timed(batch, episodes, setter):
        """(median wall s, min, max, median event ms) of `repeats` runs after a warm-up."""
        walls, mss = [], []
        for rep in range(a.repeats + 1):
            for e in episodes:
                setter(e)
            t0 = time.perf_counter()
            batch.run(a.steps)
            walls.append(time.perf_counter() - t0)
            mss.append(batch.last_ms())
        ran = [batch.episode(e)["steps_last_run"] for e in episodes]
        assert min(ran) == a.steps, f"an episode stopped early: {min(ran)} steps"
        return statistics.median(walls[1:]), min(walls[1:]), max(walls[1:]), statistics.median(mss[1:])

    def entry(t, n_episodes):
        wall, lo, hi, ms = t
        return dict(wall_s=round(wall, 6), wall_s_min=round(lo, 6), wall_s_max=round(hi, 6), event_ms=round(ms, 3),
                    episode_steps_per_s=round(n_episodes * a.steps / wall, 1), us_per_step=round(1e6 * wall / a.steps, 2))

    def dem_variant(i):
        return Z * np.float32(1.0 + 0.01 * i)

    def costmap_variant(i):
        return np.roll(cm, 3 * i, axis=1)

    res = dict(K=a.K, H=a.H, E=a.E, steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    eng = engine(a.K)
    every = range(a.E)
    for leg in a.legs:
        if leg == "plain":
            batch = _lib.Batch(eng, a.E)   # no entry point but set_episode is touched
            t = timed(batch, every, lambda e: _lib._check(
                eng.lib, eng.lib.mppi_batch_set_episode(batch.h, e, seed_state(e), 42 + e), "set_episode"))
            res[leg] = entry(t, a.E)
            batch.close()
        elif leg in ("slots1", "slots8", "dems64"):
            nd, nc = dict(slots1=(1, 1), slots8=(8, 8), dems64=(a.E, 1))[leg]
            batch = _lib.Batch(eng, a.E)
            for i in range(nd):
                batch.set_dem(i, Z if leg == "slots1" else dem_variant(i))
            for i in range(nc):
                batch.set_costmap(i, cm if leg == "slots1" else costmap_variant(i))
            t = timed(batch, every, lambda e: batch.set_episode(e, seed_state(e), 42 + e, dem=e % nd, costmap=e % nc))
            res[leg] = dict(entry(t, a.E), dem_slots=nd, costmap_slots=nc)
            batch.close()
        elif leg == "mixedk":
            ks = (a.K, a.K // 2, (a.K * 35) // 100)
            of = [ks[e % 3] for e in every]
            batch = _lib.Batch(eng, a.E)
            t = timed(batch, every, lambda e: batch.set_episode(e, seed_state(e), 42 + e, trajectories=of[e]))
            batch.close()
            parts = {}
            for k in ks:
                mine = [e for e in every if of[e] == k]
                ek = eng if k == a.K else engine(k)
                b = _lib.Batch(ek, len(mine))
                tk = timed(b, range(len(mine)), lambda j: _lib._check(
                    ek.lib, ek.lib.mppi_batch_set_episode(b.h, j, seed_state(mine[j]), 42 + mine[j]), "set_episode"))
                parts[str(k)] = dict(entry(tk, len(mine)), episodes=len(mine))
                b.close()
                if ek is not eng:
                    ek.close()
            total = sum(p["wall_s"] for p in parts.values())
            res[leg] = dict(entry(t, a.E), K_e=list(ks), separate=parts, separate_wall_s=round(total, 6),
                            mixed_over_separate_wall=round(t[0] / total, 4))
        elif leg == "score":
            out = {}
            for name in ("context", "slots"):
                batch = _lib.Batch(eng, a.E)
                if name == "slots":
                    for i in range(8):
                        batch.set_costmap(i, costmap_variant(i))
                for e in every:
                    batch.set_episode(e, seed_state(e), 42 + e, costmap=e % 8 if name == "slots" else -1)
                batch.run(a.steps)
                sw, sk = [], []
                for rep in range(a.repeats + 1):
                    t0 = time.perf_counter()
                    sc = batch.score()
                    sw.append(time.perf_counter() - t0)
                    sk.append(eng.score_ms())
                assert int(sc["rows"].min()) == a.steps
                out[name] = dict(paths=a.E, rows=a.steps, kernel_ms=round(statistics.median(sk[1:]), 4),
                                 wall_ms=round(1e3 * statistics.median(sw[1:]), 4))
                batch.close()
            res[leg] = out
        else:
            raise SystemExit(f"unknown leg {leg!r}; legs: {LEGS}")
    eng.close()
    if "plain" in res:
        for leg in ("slots1", "slots8", "dems64", "mixedk"):
            if leg in res:
                res[f"{leg}_over_plain_wall"] = round(res[leg]["wall_s"] / res["plain"]["wall_s"], 4)
    line = json.dumps(res)
    print(line)
    if a.write:
        out = os.path.join(ROOT, "profiles", "batch")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "scenes_throughput.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
