#!/usr/bin/env python3
"""Times publishing 3-D maps as pruned octree leaves (navgpu_costmap3d_export, navgpu_costmap3d_layer_update_cells) on one GPU
(needs one) beside the only route a build without them has.

  python3 tools/bench_costmap3d_publish.py [--instances 256] [--points 2000] [--reps 5] [--seed 3] [--route-instances 16] [--lib PATH] [--route-only]

Every instance is a map of the aisles map's size (tests/golden/costmap3d/aisles.bt) with DESIGN 4ac's rolling cycle: three layers,
each robot on a seeded random walk of 0..3 cells per axis and cycle, one cloud of --points points per cycle drawn from the aisles
cells in sensor range.  Legs, each timed on the host as whole calls up to the point where the stream has run dry, after a warm-up
cycle, best and median of --reps repetitions:
  cycle              roll + buffer_clouds + update of every instance
  cycle_delta        the same followed by a DELTA export of every instance
  export_full        a FULL export of every instance
  update_cells       those DELTA messages into a second handle's fed layer (AS_GIVEN), then its update
  numpy_route        per instance columns_download + free_columns_download, then the diff against the planes kept from the cycle
                     before and the prune per class in numpy - timed over the first --route-instances instances and reported per
                     instance and scaled to --instances.  It uses nothing this tool's own build adds, so --lib with the library of
                     an earlier commit and --route-only time it there.
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
SENSOR_RANGE = 3.0


def stats(ms):
    return dict(best_ms=round(min(ms), 3), median_ms=round(float(np.median(ms)), 3))


def dense(plane, sz):
    """(size_y, size_x) uint64 words -> bool [y, x, z]"""
    bits = np.unpackbits(np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape + (8,)), axis=2, bitorder="little")
    return bits[:, :, :sz].astype(bool)


def prune_dense(present, ok):
    """the maximal octree leaves of a bool volume [y, x, z] at lattice origin ok = (x, y, z): rows of (kx, ky, kz, level)"""
    span = 64
    lo = [o - o % span for o in ok]
    pad = [(ok[1] - lo[1], -(ok[1] + present.shape[0]) % span), (ok[0] - lo[0], -(ok[0] + present.shape[1]) % span), (ok[2] - lo[2], -(ok[2] + present.shape[2]) % span)]
    levels = [np.pad(present, pad)]
    while levels[-1].shape[2] > 1 and len(levels) < 7 and levels[-1].any():
        a = levels[-1]
        levels.append(a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2, a.shape[2] // 2, 2).all(axis=(1, 3, 5)))
    out = []
    for level, a in enumerate(levels):
        keep = a if level + 1 == len(levels) else a & ~np.repeat(np.repeat(np.repeat(levels[level + 1], 2, 0), 2, 1), 2, 2)
        y, x, z = np.nonzero(keep)
        out.append(np.stack([lo[0] + (x << level), lo[1] + (y << level), lo[2] + (z << level), np.full(len(x), level)], 1))
    return np.concatenate(out)


def shifted(a, dx, dy):
    """out[y, x] = a[y + dy, x + dx] inside a, else absent"""
    out = np.zeros_like(a)
    sy, sx = a.shape[:2]
    x0, x1, y0, y1 = max(0, -dx), min(sx, sx - dx), max(0, -dy), min(sy, sy - dy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=256)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--route-instances", type=int, default=16)
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
    lo = np.rint(lo / res) * res
    n, npts, reps = a.instances, a.points, a.reps
    rng = np.random.default_rng(a.seed)
    cells = np.cumsum(rng.integers(-3, 4, (n, reps + 1, 2)), 1) + rng.integers(-20, 21, (n, 1, 2))
    robots = (lo[:2] + hi[:2]) / 2 + (cells + 0.5) * res
    clouds_of = []
    for k in range(reps + 1):
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
        c.layer2d(0, 0, 0, 1, 1)

    def poses(k):
        return np.concatenate([robots[:, k], np.zeros((n, 1))], 1)

    def cycle(c, k):
        c.roll(everyone, robot_xy=robots[:, k])
        c.buffer_clouds(clouds, clouds_of[k])
        c.update(everyone, poses(k))

    out = dict(instances=n, points=npts, map=[int(s) for s in size], lib=os.path.basename(N.lib_path()))
    if not a.route_only:
        c = make()
        plain = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            cycle(c, k)
            drained(c)
            plain.append((time.perf_counter() - t0) * 1e3)
        out["cycle"] = stats(plain[1:])
        c.close()
        c = make()
        c.configure_publisher()
        b = nav.Costmap3D(n, int(size[0]), int(size[1]), int(size[2]), res, max_triangles=1, max_boxes=1 << 21, max_poses=1)
        for i in range(n):
            b.set_origin(i, lo)
        b.configure_layers([dict(kind=N.C3D_LAYER_POINT_CLOUD, max_cloud_points=1)])
        with_delta, feed, leaves = [], [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            cycle(c, k)
            msgs, values, bounds = c.export(everyone, N.C3D_EXPORT_DELTA)
            with_delta.append((time.perf_counter() - t0) * 1e3)
            leaves.append((len(values), len(bounds)))
            if k == 0:  # the warm-up's delta is every map whole: the subscriber starts from FULL exports instead, a few instances at a time
                for first in range(0, n, 32):
                    msgs, values, bounds = c.export(everyone[first:first + 32], N.C3D_EXPORT_FULL)
                    b.update_cells(msgs, np.zeros(len(msgs), np.uint32), values, bounds, cell_mode=N.C3D_CELLS_AS_GIVEN)
                b.update(everyone, poses(k))
                feed.append(0.0)
                continue
            t0 = time.perf_counter()
            verdicts = b.update_cells(msgs, np.zeros(n, np.uint32), values, bounds, cell_mode=N.C3D_CELLS_AS_GIVEN)
            b.update(everyone, poses(k))
            drained(b)
            feed.append((time.perf_counter() - t0) * 1e3)
            assert (verdicts == N.C3D_APPLIED).all()
        out["cycle_delta"] = stats(with_delta[1:])
        out["update_cells"] = stats(feed[1:])
        out["delta_leaves_per_cycle"] = [int(np.mean([v for v, _ in leaves[1:]])), int(np.mean([w for _, w in leaves[1:]]))]
        full = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            msgs, values, _ = c.export(everyone, N.C3D_EXPORT_FULL)
            full.append((time.perf_counter() - t0) * 1e3)
        out["export_full"] = stats(full[1:])
        out["full_leaves"] = int(len(values))
        c.close()
        b.close()

    # the route without the feature: raw planes over PCIe, then numpy
    r = make()
    m = min(a.route_instances, n)
    kept = [None] * m
    route, found = [], 0
    for k in range(reps + 1):
        cycle(r, k)
        drained(r)
        t0 = time.perf_counter()
        found = 0
        for i in range(m):
            lethal, nonlethal = r.columns(i)
            planes = [dense(p, int(size[2])) for p in (lethal, nonlethal, r.free_columns(i))]
            ok = [int(v) for v in np.rint(r.origin(i) / res)]
            was = kept[i]
            if was is None:
                old = [np.zeros_like(p) for p in planes]
            else:
                old = [shifted(p, ok[0] - was[1][0], ok[1] - was[1][1]) for p in was[0]]
            differs = (planes[0] ^ old[0]) | (planes[1] ^ old[1]) | (planes[2] ^ old[2])
            found += len(prune_dense(differs, ok)) + sum(len(prune_dense(p & differs, ok)) for p in planes)
            kept[i] = (planes, ok)
        route.append((time.perf_counter() - t0) * 1e3)
    s = stats(route[1:])
    out["numpy_route"] = dict(instances_timed=m, per_instance_ms=round(s["best_ms"] / m, 3), scaled_best_ms=round(s["best_ms"] * n / m, 1),
                              scaled_median_ms=round(s["median_ms"] * n / m, 1), leaves_last_cycle=found)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
