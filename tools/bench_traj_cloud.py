#!/usr/bin/env python3
"""What DWAPlanner's trajectory cloud costs: a fleet of 256 robots on 400 x 400 maps, 32 x 32 x 16 velocity samples, 20 steps, ONE
robot enabled (navgpu_planner_set_trajectory_cloud).  Reports
  - the fleet's planner cycle (navgpu_planner_cycle to a drained stream, wall time) with nobody enabled and with the one robot
    enabled, taken alternately in blocks on the same fleet (A/B/A/B...), median and spread of the block medians;
  - the read call: Fleet.trajectory_cloud (a count-only call, then scan + emit + copy), wall time, in both cost modes;
  - the bytes the read call moves against the copy rate measured on the spot: a device-to-host copy of as many bytes of the
    master grids into pageable memory.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the flagship fleet's set-up)
from navigation_amd import _lib as N  # noqa: E402


def timed_cycles(fl, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fl.planner_cycle()
        fl.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20, help="cycles per block")
    ap.add_argument("--blocks", type=int, default=5, help="A/B blocks of each kind")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robot", type=int, default=0)
    args = ap.parse_args()
    import navigation_amd as nav
    fl, insts, cfg = bench.build_fleet(nav, args.robots, args.size, 0)
    fl.update_map()
    timed_cycles(fl, args.warmup)
    off, on = [], []
    for _ in range(args.blocks):
        fl.set_trajectory_cloud(False, first=args.robot, count=1)
        off.append(timed_cycles(fl, args.steps))
        fl.set_trajectory_cloud(True, first=args.robot, count=1)
        timed_cycles(fl, 1)  # (the records are allocated by the first cycle)
        on.append(timed_cycles(fl, args.steps))
    read = {}
    for mode in (True, False):
        t = []
        for i in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            cloud = fl.trajectory_cloud(args.robot, reference_costs=mode)
            if i >= args.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        read[mode] = (float(np.median(t)), float(np.min(t)), float(np.max(t)), len(cloud))
    n_bytes = read[False][3] * 28
    per_robot = args.size * args.size
    k = max(1, min(args.robots, (n_bytes + per_robot - 1) // per_robot))
    t = []
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        fl.download(N.GRID_MASTER, first=0, count=k)
        if i >= args.warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    copy_ms, copy_bytes = float(np.median(t)), k * per_robot
    terms = fl.sample_terms(args.robot)
    out = {"robots": args.robots, "size": args.size, "slots": int(len(terms)), "scored": int((terms["status"] == 1).sum()),
           "timing": f"wall, medians of {args.steps}-cycle blocks, {args.blocks} blocks of each kind alternating; read call: median (min, max) of {args.steps}",
           "cycle_nobody_enabled_ms": round(float(np.median(off)), 4), "cycle_nobody_enabled_spread_ms": [round(min(off), 4), round(max(off), 4)],
           "cycle_one_enabled_ms": round(float(np.median(on)), 4), "cycle_one_enabled_spread_ms": [round(min(on), 4), round(max(on), 4)],
           "read_reference_costs_ms": [round(v, 4) for v in read[True][:3]], "read_reference_costs_points": read[True][3],
           "read_full_costs_ms": [round(v, 4) for v in read[False][:3]], "read_full_costs_points": read[False][3],
           "read_full_costs_bytes": n_bytes, "copy_same_bytes_ms": round(copy_ms, 4), "copy_rate_gb_s": round(copy_bytes / copy_ms / 1e6, 3),
           "read_full_costs_effective_gb_s": round(n_bytes / read[False][0] / 1e6, 3)}
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
