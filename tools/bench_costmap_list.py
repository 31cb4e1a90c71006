#!/usr/bin/env python3
"""Time the costmap update (stage + update + a wait) of some robots of a fleet, for 256 robots at the benchmark's shape (bench.py's fleet:
400 x 400 maps, static + obstacle + inflation layers, one 720-beam scan per robot).

  fixed window    every third robot, alternating robots, one robot and everyone - through the listed calls (navgpu_costmap_stage_list +
                  navgpu_costmap_update_list: one upload, one launch of each kernel) and through the range calls, contiguous run by
                  contiguous run (one stage and one update per run).  A build without the listed calls reports the range figures only.
  rolling window  (obstacle + inflation layers, the robots moving 0.1 m back and forth so that every update shifts) the whole-fleet
                  stage + update, which is all the range calls take, and listed updates of 1, 32, 86 and 256 robots.

The range figures are public calls every build has: run the tool from a checkout of the parent commit as well (copy this file into its
tools/) and set the JSON lines side by side, runs interleaved.  Medians of --steps calls after --warmup, wall ms of stage + update + sync."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from navigation_amd import _lib as N  # noqa: E402


def median_ms(call, steps, warmup):
    t = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        call(i)
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return round(float(np.median(t)), 4)


def runs_of(robots):
    runs = []
    for r in robots:
        if runs and runs[-1][0] + runs[-1][1] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    return [tuple(r) for r in runs]


def pack(obs):
    """pre-marshalled arguments of a stage call: (Observation array, count, packed points)"""
    arr = (N.Observation * max(1, len(obs)))()
    pts, off = [], 0
    for k, o in enumerate(obs):
        p = np.ascontiguousarray(o["points"], np.float32).reshape(-1, 3)
        org = o["origin"]
        arr[k] = N.Observation(o["instance"], off, len(p), N.OBS_MARKING | N.OBS_CLEARING, org[0], org[1], org[2], o["obstacle_range"], o["raytrace_range"])
        pts.append(p)
        off += len(p)
    return arr, len(obs), np.ascontiguousarray(np.concatenate(pts), np.float32)


class Selection:
    """some robots of a fleet with everything their stage calls hand over ready, in two pose sets that alternate step by step"""

    def __init__(self, fl, robots, poses, obs, wiggle):
        self.fl, self.robots = fl, np.asarray(robots, np.uint32)
        self.listed = hasattr(fl, "update_map_list")
        self.runs = runs_of(list(robots))
        self.poses = [np.ascontiguousarray(poses[robots] + np.array([d, -d, 0.0])) for d in (0.0, wiggle)]
        self.packed = pack([obs[i] for i in robots])
        self.run_inputs = []
        for first, count in self.runs:
            k = list(robots).index(first)
            self.run_inputs.append((first, count, [p[k:k + count] for p in self.poses], pack([obs[i] for i in robots[k:k + count]])))

    def by_list(self, step):
        arr, n, pts = self.packed
        self.fl.stage_observations_list_raw(self.robots, self.poses[step & 1], arr, n, pts)
        self.fl.update_map_list(self.robots)
        self.fl.sync()

    def by_runs(self, step):
        for first, count, poses, (arr, n, pts) in self.run_inputs:
            self.fl.stage_observations_raw(poses[step & 1], arr, n, pts, first=first)
        for first, count, _, _ in self.run_inputs:
            self.fl.update_map(first, count)
        self.fl.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", choices=["fixed", "rolling", "both"], default="both")
    args = ap.parse_args()
    import bench
    import navigation_amd as nav
    from navigation_amd import synth
    n = args.robots
    fl, insts, _ = bench.build_fleet(nav, n, args.size, seed0=0)
    poses, obs = fl._bench_host_inputs[0], fl._bench_host_inputs[1]
    out = {"robots": n, "size": args.size, "lib": os.path.basename(N.lib_path()), "listed_calls": hasattr(fl, "update_map_list"),
           "timing": "median wall ms of stage + update + sync"}
    everyone = list(range(n))
    selections = (("every_third", everyone[::3]), ("alternating", everyone[::2]), ("one", [n // 2]), ("everyone", everyone))
    if args.leg in ("fixed", "both"):
        fl.update_map()
        fl.sync()
        for name, robots in selections:
            s = Selection(fl, robots, poses, obs, 0.0)
            row = {"robots": len(robots), "runs": len(s.runs), "by_runs_ms": median_ms(s.by_runs, args.steps, args.warmup)}
            if s.listed:
                row["listed_ms"] = median_ms(s.by_list, args.steps, args.warmup)
                row["by_runs_again_ms"] = median_ms(s.by_runs, args.steps, args.warmup)
            out["fixed_" + name] = row
    fl.close()
    if args.leg in ("rolling", "both"):
        fp = synth.FOOTPRINT
        rl = nav.Fleet(n, args.size, args.size, synth.RES, layers=N.LAYER_OBSTACLE | N.LAYER_INFLATION, max_points=720, max_observations=1,
                       max_plan=200, max_footprint=8, max_sim_steps=24, rolling_window=True)
        rl.configure_obstacle()
        rl.set_footprint(fp)
        rl.configure_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, synth.inscribed_radius(fp))
        whole = Selection(rl, everyone, poses, obs, 0.1)
        out["rolling_whole_fleet_range_ms"] = median_ms(whole.by_runs, args.steps, args.warmup)  # (one run: the whole fleet)
        if whole.listed:
            for k in (1, 32, 86, 256):
                if k > n:
                    continue
                robots = everyone[::max(1, n // k)][:k] if k > 1 else [n // 2]
                s = Selection(rl, robots, poses, obs, 0.1)
                out["rolling_listed_%d_ms" % k] = median_ms(s.by_list, args.steps, args.warmup)
            out["rolling_whole_fleet_range_again_ms"] = median_ms(whole.by_runs, args.steps, args.warmup)
        rl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
