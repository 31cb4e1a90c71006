#!/usr/bin/env python3
"""Times navgpu_costmap3d_query and navgpu_costmap3d_footprint_costs on one GPU (needs one).

  python3 tools/bench_costmap3d.py [--instances 256] [--poses 64] [--footprint-poses 4096] [--reps 5] [--seed 3]

Every instance holds the aisles map (tests/golden/costmap3d/aisles.bt), the mesh is the reference's test robot.  Three legs, each a
whole call - upload, launch set, read-back - timed on the host after a warm-up call, best and median of --reps:
  collision   one path of --poses poses per instance, collision mode
  distance    the same paths, distance mode without a limit
  footprint   --footprint-poses (x, y, theta) poses per instance through footprint_costs
Paths are random walks over the map at z = 0 (seeded).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import navigation_amd as nav  # noqa: E402
from navigation_amd.costmap3d import load_stl, read_octomap_bt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(best_ms=round(min(ms), 3), median_ms=round(float(np.median(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--footprint-poses", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    lo = (t["centres"] - 0.5 * t["sizes"][:, None]).min(0)
    hi = (t["centres"] + 0.5 * t["sizes"][:, None]).max(0)
    size = np.rint((hi - lo) / t["res"]).astype(int)
    n_max = a.instances * max(a.poses, a.footprint_poses)
    c = nav.Costmap3D(a.instances, int(size[0]), int(size[1]), int(size[2]), t["res"], max_triangles=32, max_boxes=16384, max_poses=n_max)
    c.set_mesh(*load_stl(os.path.join(GOLDEN, "test_robot.stl")))
    for i in range(a.instances):
        c.set_origin(i, lo)
        c.set_boxes(i, t["centres"], t["sizes"], t["classes"])
    rng = np.random.default_rng(a.seed)

    def walks(n):  # (instances * n, 3) x, y, theta: a start anywhere on the map, steps of about a cell and a few degrees
        start = np.stack([rng.uniform(lo[0], hi[0], a.instances), rng.uniform(lo[1], hi[1], a.instances), rng.uniform(-np.pi, np.pi, a.instances)], 1)
        steps = np.concatenate([rng.normal(0.0, t["res"], (a.instances, n, 2)), rng.normal(0.0, 0.05, (a.instances, n, 1))], 2)
        return (start[:, None, :] + np.cumsum(steps, 1)).reshape(-1, 3)

    def as_poses(xyth):
        p = np.zeros((len(xyth), 7))
        p[:, 0], p[:, 1], p[:, 5], p[:, 6] = xyth[:, 0], xyth[:, 1], np.sin(xyth[:, 2] / 2), np.cos(xyth[:, 2] / 2)
        return p

    path = as_poses(walks(a.poses))
    runs = [(i, i * a.poses, a.poses) for i in range(a.instances)]
    out = dict(instances=a.instances, poses=a.poses, footprint_poses=a.footprint_poses, map=[int(s) for s in size], occupied_cells=33 * 8 + 10421,
               triangles=28)
    costs, _ = c.query(path, runs=runs, mode=nav._lib.C3D_COLLISION_ONLY)
    out["colliding_fraction"] = round(float((costs < 0).mean()), 3)
    out["collision"] = timed(lambda: c.query(path, runs=runs, mode=nav._lib.C3D_COLLISION_ONLY), a.reps)
    out["distance"] = timed(lambda: c.query(path, runs=runs, mode=nav._lib.C3D_DISTANCE), a.reps)
    xyth = walks(a.footprint_poses)
    fruns = [(i, i * a.footprint_poses, a.footprint_poses) for i in range(a.instances)]
    out["footprint"] = timed(lambda: c.footprint_costs(xyth, runs=fruns), a.reps)
    for leg, n in (("collision", len(path)), ("distance", len(path)), ("footprint", len(xyth))):
        out[leg]["us_per_pose"] = round(out[leg]["best_ms"] * 1e3 / n, 3)
    c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
