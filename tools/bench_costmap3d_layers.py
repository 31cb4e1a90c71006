#!/usr/bin/env python3
"""Times the layered costmap_3d update (navgpu_costmap3d_buffer_clouds, _update, _layer2d_update_costs) on one GPU (needs one).

  python3 tools/bench_costmap3d_layers.py [--instances 256] [--points 20000] [--reps 5] [--seed 3] [--lib PATH] [--ab]

Every instance is a map of the aisles map's size (tests/golden/costmap3d/aisles.bt) with three layers: a static grid at the
floor, a point-cloud layer, a clearing cylinder.  Per cycle each instance gets one cloud of --points points, drawn from the aisles
cells inside a sensor-range box round a pose on a seeded random walk and jittered inside their cells.  Legs, each a whole call
timed on the host after a warm-up cycle, best and median of --reps cycles (every cycle has its own clouds and poses):
  buffer_clouds   all instances' clouds in one call
  update          all instances in one call
  cycle           both together
  update_costs_2d the projected layer into the master grids of a fleet of that size, whole maps, updateWithMax
  set_boxes_route what the library offered before for the same clouds: the host turns each cloud into its cell list with
                  numpy and calls set_boxes(REPLACE) per instance (same box, same run)
--lib names another build of the library.  --ab runs this script twice more as child processes on the tool build
(make -C navigation_amd/csrc c3d-layers-ab), with and without NAVGPU_C3D_ALL_TILES=1 - the plain full-volume pass of the swap and
the combine against the tile-skipping one - and adds their legs.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import navigation_amd as nav  # noqa: E402
from navigation_amd import _lib as N  # noqa: E402
from navigation_amd.costmap3d import read_octomap_bt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")
SENSOR_RANGE = 3.0  # half the edge of the box round the pose, metres


def stats(ms):
    return dict(best_ms=round(min(ms), 3), median_ms=round(float(np.median(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    if a.lib:
        N.lib_path = lambda: os.path.abspath(a.lib)
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    res = t["res"]
    half = 0.5 * t["sizes"][:, None]
    lo, hi = (t["centres"] - half).min(0), (t["centres"] + half).max(0)
    size = np.rint((hi - lo) / res).astype(int)
    n, npts = a.instances, a.points
    rng = np.random.default_rng(a.seed)

    c = nav.Costmap3D(n, int(size[0]), int(size[1]), int(size[2]), res, max_triangles=1, max_boxes=max(npts, 1), max_poses=1)
    for i in range(n):
        c.set_origin(i, lo)
    c.configure_layers([dict(kind=N.C3D_LAYER_STATIC_2D, height=float(lo[2]), lethal_cost_threshold=100, combination_method=N.C3D_COMBINE_OVERWRITE),
                        dict(kind=N.C3D_LAYER_POINT_CLOUD, max_cloud_points=n * npts, combination_method=N.C3D_COMBINE_MAXIMUM),
                        dict(kind=N.C3D_LAYER_CYLINDER_CLEARING, radius=0.5)])
    floor = np.zeros((size[1], size[0]), np.int8)
    for i in range(n):
        c.set_static_grid(i, 0, floor, lo[0], lo[1])

    # the walks: a start anywhere on the map, steps of a few cells; a cycle's cloud per instance from the cells in range
    start = np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n)], 1)
    steps = rng.normal(0.0, 4 * res, (n, a.reps + 1, 2))
    walk = np.clip(start[:, None, :] + np.cumsum(steps, 1), lo[:2], hi[:2])
    cycles = []
    for k in range(a.reps + 1):
        pts = np.zeros((n, npts, 3), np.float32)
        for i in range(n):
            near = np.flatnonzero(np.all(np.abs(t["centres"][:, :2] - walk[i, k]) <= SENSOR_RANGE, axis=1))
            near = near if len(near) else np.arange(len(t["centres"]))
            pick = near[rng.integers(0, len(near), npts)]
            pts[i] = t["centres"][pick] + (rng.random((npts, 3)) - 0.5) * 0.98 * t["sizes"][pick, None]
        poses = np.concatenate([walk[:, k], np.zeros((n, 1))], 1)
        cycles.append((pts.reshape(-1, 3), poses))
    clouds = [(i, 1, i * npts, npts) for i in range(n)]
    everyone = np.arange(n, dtype=np.uint32)

    legs = dict(buffer_clouds=[], update=[], cycle=[])
    touched = []
    for k, (pts, poses) in enumerate(cycles):
        t0 = time.perf_counter()
        clipped = c.buffer_clouds(clouds, pts)
        t1 = time.perf_counter()
        bounds = c.update(everyone, poses)
        t2 = time.perf_counter()
        assert not clipped.any()
        if k:  # (cycle 0 is the warm-up and the full update)
            legs["buffer_clouds"].append((t1 - t0) * 1e3)
            legs["update"].append((t2 - t1) * 1e3)
            legs["cycle"].append((t2 - t0) * 1e3)
            touched.append(float(np.mean((bounds[:, 2] - bounds[:, 0]) * (bounds[:, 3] - bounds[:, 1]) / ((hi[0] - lo[0]) * (hi[1] - lo[1])))))
    out = dict(instances=n, points=npts, map=[int(s) for s in size], lib=os.path.basename(N.lib_path()),
               all_tiles=bool(os.environ.get("NAVGPU_C3D_ALL_TILES")), bounds_box_fraction=round(float(np.mean(touched)), 3))
    out.update({name: stats(ms) for name, ms in legs.items()})
    lethal = c.layer_columns(0, 1)[0]  # the cloud layer of the last cycle

    fl = nav.Fleet(n, int(size[0]), int(size[1]), res)
    boxes = np.tile(np.array([0, 0, size[0], size[1]], np.int32), (n, 1))
    ms = []
    for k in range(a.reps + 1):
        t0 = time.perf_counter()
        c.update_costs_2d(fl, everyone, boxes, True)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["update_costs_2d"] = stats(ms[1:])
    fl.close()
    c.close()

    if not a.skip_baseline:
        b = nav.Costmap3D(n, int(size[0]), int(size[1]), int(size[2]), res, max_triangles=1, max_boxes=max(npts, 1), max_poses=1)
        for i in range(n):
            b.set_origin(i, lo)
        ms = []
        for k, (pts, _) in enumerate(cycles):
            t0 = time.perf_counter()
            for i in range(n):
                cells = np.unique(np.floor((pts[i * npts:(i + 1) * npts].astype(np.float64) - lo) / res).astype(np.int64), axis=0)
                b.set_boxes(i, lo + (cells + 0.5) * res, res)
            b.columns(0)  # (set_boxes only queues: wait for the last one)
            ms.append((time.perf_counter() - t0) * 1e3)
        out["set_boxes_route"] = stats(ms[1:])
        out["same_cells_as_the_cloud_layer_instance0"] = bool(np.array_equal(b.columns(0)[0], lethal))
        b.close()

    if a.ab:
        ab = os.path.join(os.path.dirname(nav.lib_path()), "libnavgpu_c3d_ab.so")
        for name, env in (("ab_tile_skipping", {}), ("ab_all_tiles", {"NAVGPU_C3D_ALL_TILES": "1"})):
            cmd = [sys.executable, os.path.abspath(__file__), "--instances", str(n), "--points", str(npts), "--reps", str(a.reps), "--seed", str(a.seed),
                   "--lib", ab, "--skip-baseline"]
            r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, check=True)
            child = json.loads(r.stdout.strip().splitlines()[-1])
            out[name] = {k: child[k] for k in ("buffer_clouds", "update", "cycle", "all_tiles")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
