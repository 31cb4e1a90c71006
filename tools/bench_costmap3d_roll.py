#!/usr/bin/env python3
"""Times rolling 3-D maps (navgpu_costmap3d_roll) on one GPU (needs one) beside the route a build without it has.

  python3 tools/bench_costmap3d_roll.py [--instances 256] [--points 20000] [--reps 5] [--seed 3] [--lib PATH] [--route-only]

Every instance is a map of the aisles map's size (tests/golden/costmap3d/aisles.bt) with three layers: a static grid at the floor,
a point-cloud layer, a clearing cylinder.  Each robot is on a seeded random walk that moves its window by 0..3 cells per axis and
cycle, and gets one cloud of --points points per cycle, drawn from the aisles cells in sensor range of it and jittered inside
their cells.  Legs, each timed on the host as whole calls up to the point where the stream has run dry, after a warm-up cycle,
best and median of --reps cycles:
  roll_all / roll_every_4th / roll_one   navgpu_costmap3d_roll alone: every instance, every fourth, one
  cycle_rolling      roll + buffer_clouds + update of every instance
  cycle_fixed        buffer_clouds + update, the windows standing still (DESIGN 4ab's cycle)
  cycle_reset_route  the same end state without the roll: per moved instance set_origin, reset and set_static_grid, then
                     buffer_clouds + update of every instance (a full-volume update and a full re-projection each).  It uses
                     nothing this tool's own build adds, so --lib with the library of an earlier commit and --route-only time
                     it there.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import navigation_amd as nav  # noqa: E402
from navigation_amd import _lib as N  # noqa: E402
from navigation_amd.costmap3d import read_octomap_bt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")
SENSOR_RANGE = 3.0  # half the edge of the box round the robot, metres


def stats(ms):
    return dict(best_ms=round(min(ms), 3), median_ms=round(float(np.median(ms)), 3))


def window_key(robot, size, res):
    """the first key of the window round a robot coordinate (include/navgpu_costmap3d_rolling.h, NAVGPU_C3D_ROLL_CENTRE)"""
    w = np.float64(np.float32(np.float64(size) * np.float64(res)))
    m = np.float32(np.float64(robot) - w / np.float64(2.0))
    return int(np.floor(np.float64(m) * (np.float64(1.0) / np.float64(res))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--route-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        N.lib_path = lambda: os.path.abspath(a.lib)
        if a.route_only:  # an earlier commit's library: bind what it exports (the route needs none of the rest)
            import ctypes
            probe = ctypes.CDLL(N.lib_path())
            N.SYMBOLS = [s for s in N.SYMBOLS if hasattr(probe, s[0])]
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    res = t["res"]
    half = 0.5 * t["sizes"][:, None]
    lo, hi = (t["centres"] - half).min(0), (t["centres"] + half).max(0)
    size = np.rint((hi - lo) / res).astype(int)
    lo = np.rint(lo / res) * res  # an aligned origin
    n, npts = a.instances, a.points
    rng = np.random.default_rng(a.seed)

    # the walks, in cells: a start round the map's centre, then 0..3 cells per axis and cycle either way
    cells = np.cumsum(rng.integers(-3, 4, (n, a.reps + 1, 2)), 1) + rng.integers(-20, 21, (n, 1, 2))
    robots = (lo[:2] + hi[:2]) / 2 + (cells + 0.5) * res  # [n][cycle][2]
    clouds_of = []
    for k in range(a.reps + 1):
        pts = np.zeros((n, npts, 3), np.float32)
        for i in range(n):
            near = np.flatnonzero(np.all(np.abs(t["centres"][:, :2] - robots[i, k]) <= SENSOR_RANGE, axis=1))
            near = near if len(near) else np.arange(len(t["centres"]))
            pick = near[rng.integers(0, len(near), npts)]
            pts[i] = t["centres"][pick] + (rng.random((npts, 3)) - 0.5) * 0.98 * t["sizes"][pick, None]
        clouds_of.append(pts.reshape(-1, 3))
    clouds = [(i, 1, i * npts, npts) for i in range(n)]
    everyone = np.arange(n, dtype=np.uint32)
    floor = np.zeros((size[1], size[0]), np.int8)

    def make():
        c = nav.Costmap3D(n, int(size[0]), int(size[1]), int(size[2]), res, max_triangles=1, max_boxes=1, max_poses=1)
        for i in range(n):
            c.set_origin(i, lo)
        c.configure_layers([dict(kind=N.C3D_LAYER_STATIC_2D, height=float(lo[2]), lethal_cost_threshold=100, combination_method=N.C3D_COMBINE_OVERWRITE),
                            dict(kind=N.C3D_LAYER_POINT_CLOUD, max_cloud_points=n * npts, combination_method=N.C3D_COMBINE_MAXIMUM),
                            dict(kind=N.C3D_LAYER_CYLINDER_CLEARING, radius=0.5)])
        for i in range(n):
            c.set_static_grid(i, 0, floor, lo[0], lo[1])
        return c

    def drained(c):
        c.layer2d(0, 0, 0, 1, 1)  # one byte back: the stream has run dry

    def poses(k):
        return np.concatenate([robots[:, k], np.zeros((n, 1))], 1)

    out = dict(instances=n, points=npts, map=[int(s) for s in size], lib=os.path.basename(N.lib_path()))
    if not a.route_only:
        c = make()
        cycle, moved = [], []
        for k in range(a.reps + 1):
            t0 = time.perf_counter()
            shifts = c.roll(everyone, robot_xy=robots[:, k])
            c.buffer_clouds(clouds, clouds_of[k])
            c.update(everyone, poses(k))
            drained(c)
            if k:  # (cycle 0 is the warm-up, the jump to the robots and the full update)
                cycle.append((time.perf_counter() - t0) * 1e3)
                moved.append(float(np.mean(np.any(shifts != 0, axis=1))))
        out["cycle_rolling"] = stats(cycle)
        out["moved_fraction"] = round(float(np.mean(moved)), 3)
        fixed = []
        for k in range(a.reps + 1):
            t0 = time.perf_counter()
            c.buffer_clouds(clouds, clouds_of[k])
            c.update(everyone, poses(k))
            drained(c)
            fixed.append((time.perf_counter() - t0) * 1e3)
        out["cycle_fixed"] = stats(fixed[1:])
        # the roll alone: every listed robot one cell on in x and y each time, so every listed instance moves
        for name, listed in (("roll_all", everyone), ("roll_every_4th", everyone[::4]), ("roll_one", everyone[:1])):
            ms = []
            at = robots[listed, -1].copy()
            for k in range(a.reps + 1):
                at += res * np.array([1 + k % 3, 1 + (k + 1) % 3])
                drained(c)
                t0 = time.perf_counter()
                shifts = c.roll(listed, robot_xy=at)
                drained(c)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert np.all(shifts != 0)
            out[name] = stats(ms[1:])
        c.close()

    b = make()
    windows = np.array([[[window_key(robots[i, k, axis], size[axis], res) for axis in range(2)] for i in range(n)] for k in range(a.reps + 1)])
    keys = windows[0]
    route = []
    for k in range(a.reps + 1):
        new = windows[k]
        t0 = time.perf_counter()
        for i in np.flatnonzero(np.any(new != keys, axis=1) | (k == 0)):
            b.set_origin(i, [new[i, 0] * res, new[i, 1] * res, lo[2]])
            b.reset([i])
            b.set_static_grid(i, 0, floor, new[i, 0] * res, new[i, 1] * res)
        keys = new
        b.buffer_clouds(clouds, clouds_of[k])
        b.update(everyone, poses(k))
        drained(b)
        route.append((time.perf_counter() - t0) * 1e3)
    out["cycle_reset_route"] = stats(route[1:])
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
