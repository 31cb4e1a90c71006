#!/usr/bin/env python3
"""Time k_footprint_cost under its two users, for 256 robots on 400 x 400 maps with a 4-vertex footprint:
  rotate  navgpu_rotate_recovery_step, the first pass of a run: one sweep of pi / 0.017 = 185 headings per robot
  carrot  navgpu_carrot_plan: 100 candidates per plan along random start-goal lines
Per launch: device time between two HIP events around the kernel (the library's profile brackets), after warm-up, median of
--steps launches; and the host's wall time for the whole call (query upload, launch, result download, synchronise).  Against
the CPU oracle's footprint_cost on the same queries (--oracle-robots robots' worth, scaled to the fleet; one Python call per
query on a 64 x 64 crop of the map around the pose, so the figure carries ~5 us of call overhead per query), whose answers
are also compared with the device's.

The other work split - one lane per query walking the whole outline - is a build of the same kernel behind
-DNAVGPU_FOOTPRINT_LANE_PER_QUERY:  make -C navigation_amd/csrc footprint-ab  links it into navigation_amd/libnavgpu_lpq.so
beside the shipped library, and  --ab  then measures both, each in a process of its own, and prints one JSON line with the
two results side by side.  --lib measures one library of the caller's choice."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navigation_amd import _lib as N  # noqa: E402

RES = 0.05
FOOTPRINT = [[0.25, 0.2], [-0.25, 0.2], [-0.25, -0.2], [0.25, -0.2]]
CROP = 32  # cells either side of the pose in the oracle's crop


def make_maps(rs, n_robots, n):
    g = np.zeros((n_robots, n, n), np.uint8)
    g[rs.random_sample(g.shape) < 0.002] = 254
    near = np.zeros_like(g, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= np.roll(np.roll(g == 254, dy, 1), dx, 2)
    g[near & (g == 0)] = 128
    return g


def host_cost(orc, grid, x, y, th):
    """the oracle on a crop around the pose (same cells, same answer while the footprint stays inside the crop)"""
    n = grid.shape[0]
    cx, cy = int(x / RES), int(y / RES)
    if x < 0 or y < 0 or cx >= n or cy >= n:
        return -1.0
    x0, y0 = max(cx - CROP, 0), max(cy - CROP, 0)
    sub = grid[y0:cy + CROP, x0:cx + CROP]
    if x0 > 0 and y0 > 0 and cx + CROP <= n and cy + CROP <= n:
        return orc.footprint_cost(sub, RES, 0.0, 0.0, x - x0 * RES, y - y0 * RES, th, FOOTPRINT, False)
    return orc.footprint_cost(grid, RES, 0.0, 0.0, x, y, th, FOOTPRINT, False)  # near the border: the whole map


def timed(fl, steps, warmup, call):
    dev, wall = [], []
    for i in range(warmup + steps):
        fl.profile_reset()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        ms, n = fl.profile_read()["k_footprint_cost"]
        assert n == 1
        if i >= warmup:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    return round(float(np.median(dev)), 4), round(float(np.median(wall)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--oracle-robots", type=int, default=8)
    ap.add_argument("--lib", default=None, help="another build of libnavgpu.so (the lane-per-query split)")
    ap.add_argument("--ab", action="store_true", help="both splits, the shipped library and libnavgpu_lpq.so (make footprint-ab)")
    args = ap.parse_args()
    if args.ab:
        lpq = os.path.join(os.path.dirname(N.lib_path()), "libnavgpu_lpq.so")
        if not os.path.exists(lpq):
            sys.exit(f"{lpq} is missing: make -C navigation_amd/csrc footprint-ab")
        base = [sys.executable, os.path.abspath(__file__), "--robots", str(args.robots), "--size", str(args.size), "--steps", str(args.steps),
                "--warmup", str(args.warmup), "--oracle-robots", str(args.oracle_robots)]
        res = {}
        for name, extra in (("edge_per_lane", []), ("query_per_lane", ["--lib", lpq])):
            r = subprocess.run(base + extra, stdout=subprocess.PIPE, text=True, check=True)
            res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        res["rotate_faster"] = min(("edge_per_lane", "query_per_lane"), key=lambda k: res[k]["rotate_device_ms"])
        print(json.dumps(res))
        return
    if args.lib:
        N.lib_path = lambda: os.path.abspath(args.lib)
    import navigation_amd as nav
    nR, n = args.robots, args.size
    rs = np.random.RandomState(0)
    maps = make_maps(rs, nR, n)
    fl = nav.Fleet(nR, n, n, RES, layers=N.LAYER_OBSTACLE, max_footprint=4)
    fl.set_footprint(FOOTPRINT)
    fl.upload(N.GRID_MASTER, maps)
    fl.configure_rotate_recovery()  # the reference's defaults
    fl.profile_select(["k_footprint_cost"])
    fl.profile(True)
    out = {"robots": nR, "size": n, "lib": os.path.basename(N.lib_path()), "timing": "median; device = HIP events around the kernel, wall = the whole call"}

    # ---- rotate: the first pass of a run, every robot somewhere in the middle of its map
    poses = np.column_stack([rs.uniform(2.0, n * RES - 2.0, nR), rs.uniform(2.0, n * RES - 2.0, nR), rs.uniform(-math.pi, math.pi, nR)])
    states = (N.RotateRecoveryState * nR)()

    def rotate():
        C.memset(states, 0, C.sizeof(states))
        rotate.result = fl.rotate_recovery_step(poses, states)
    out["rotate_device_ms"], out["rotate_wall_ms"] = timed(fl, args.steps, args.warmup, rotate)
    status = rotate.result[1]
    sim, angles = 0.0, []  # the first pass's sweep: dist_left = pi (rotate_recovery.cpp:117-129)
    while sim < math.pi:
        angles.append(sim)
        sim += 0.017
    out["rotate_queries"] = len(angles) * nR
    assert all(s.swept == len(angles) or status[k] == N.ROTATE_BLOCKED for k, s in enumerate(states))
    out["rotate_blocked"] = int((status == N.ROTATE_BLOCKED).sum())
    # the same queries through navgpu_footprint_cost (costs downloaded too) and through the oracle
    runs = [np.column_stack([np.full(len(angles), p[0]), np.full(len(angles), p[1]), p[2] + np.array(angles)]) for p in poses]
    out["rotate_query_device_ms"], out["rotate_query_wall_ms"] = timed(fl, args.steps, args.warmup, lambda: fl.footprint_cost(runs, allow_unknown=False))
    costs, first_illegal = fl.footprint_cost(runs, allow_unknown=False)
    assert all((first_illegal[k] >= 0) == (status[k] == N.ROTATE_BLOCKED) for k in range(nR))
    if args.oracle_robots:
        from oracle import pyoracle as orc
        orc.lib()
        k_or = min(args.oracle_robots, nR)
        t0 = time.perf_counter()
        want = [np.array([host_cost(orc, maps[k], *q) for q in runs[k]]) for k in range(k_or)]
        dt = time.perf_counter() - t0
        out["rotate_oracle_ms_scaled"] = round(dt * 1e3 * nR / k_or, 1)
        out["rotate_oracle_mismatches"] = int(sum((want[k] != costs[k]).sum() for k in range(k_or)))

    # ---- carrot: random start-goal lines
    starts = np.column_stack([rs.uniform(1.0, n * RES - 1.0, nR), rs.uniform(1.0, n * RES - 1.0, nR), rs.uniform(-math.pi, math.pi, nR)])
    goals = np.column_stack([rs.uniform(1.0, n * RES - 1.0, nR), rs.uniform(1.0, n * RES - 1.0, nR), rs.uniform(-math.pi, math.pi, nR)])

    def carrot():
        carrot.result = fl.carrot_plan(starts, goals, allow_unknown=False)
    out["carrot_device_ms"], out["carrot_wall_ms"] = timed(fl, args.steps, args.warmup, carrot)
    targets, found = carrot.result
    out["carrot_found"] = int((found > 0).sum())
    out["carrot_mean_tried"] = round(float(found[found > 0].mean()), 2) if (found > 0).any() else 0.0
    if args.oracle_robots:
        k_or = min(args.oracle_robots, nR)
        norm = lambda a: N.lib().navgpu_shortest_angular_distance(0.0, a)  # noqa: E731
        t0 = time.perf_counter()
        bad = 0
        for k in range(k_or):  # the whole candidate list, as the device evaluates it
            s, g = starts[k], goals[k]
            dyaw = norm(g[2] - s[2])
            scale, first = 1.0, 0
            i = 0
            while not scale < 0:
                i += 1
                c = host_cost(orc, maps[k], s[0] + scale * (g[0] - s[0]), s[1] + scale * (g[1] - s[1]), norm(s[2] + scale * dyaw))
                if c >= 0 and not first:
                    first = i
                scale -= 0.01
            bad += int(first != found[k])
        dt = time.perf_counter() - t0
        out["carrot_oracle_ms_scaled"] = round(dt * 1e3 * nR / k_or, 1)
        out["carrot_oracle_mismatches"] = bad
    fl.profile(False)
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
