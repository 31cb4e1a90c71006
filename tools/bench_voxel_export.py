#!/usr/bin/env python3
"""Time navgpu_voxel_points(MARKED) for 64 robots on 1000 x 1000 voxel maps (z_voxels 10) after one update with a laser
scan per robot, against the same answer made on the host: navgpu_grid_download(NAVGPU_GRID_VOXEL) plus a vectorised numpy
classification of the columns.  Per call, after warm-up, median of --steps: the device time between HIP events around the
count / scan / emit launches (the library's profile brackets, summed over the call) and the host's wall time for the whole
call (both passes of Fleet.voxel_points: count, then emit and download).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navigation_amd import _lib as N  # noqa: E402
from navigation_amd import synth  # noqa: E402

Z_VOXELS, ORIGIN_Z, Z_RES = 10, 0.0, 0.2


def host_marked_points(fl):
    """download + classify on the host: marked = hi & lo & zmask per column, then its set bits in ascending z"""
    vox = fl.download(N.GRID_VOXEL)
    org = fl.origins()
    zmask = np.uint32((1 << Z_VOXELS) - 1)
    out = []
    for k in range(fl.n):
        bits = (vox[k] >> np.uint32(16)) & vox[k] & zmask
        my, mx = np.nonzero(bits)
        b = bits[my, mx]
        z = np.arange(Z_VOXELS, dtype=np.uint32)
        on = ((b[:, None] >> z) & np.uint32(1)).astype(bool)
        col, mz = np.nonzero(on)
        xyz = np.stack([org[k, 0] + (mx[col] + 0.5) * fl.res, org[k, 1] + (my[col] + 0.5) * fl.res, ORIGIN_Z + (mz + 0.5) * Z_RES], axis=1)
        out.append(xyz.astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import navigation_amd as nav
    nR, n = args.robots, args.size
    fl = nav.Fleet(nR, n, n, synth.RES, layers=N.LAYER_VOXEL | N.LAYER_INFLATION, track_unknown=True, max_points=1440, max_observations=1)
    fl.configure_obstacle(z_voxels=Z_VOXELS, origin_z=ORIGIN_Z, z_resolution=Z_RES, max_obstacle_height=2.0)
    fl.set_footprint(synth.FOOTPRINT5)
    fl.configure_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, synth.inscribed_radius(synth.FOOTPRINT5))
    worlds = [synth.make_instance(n, 50 + i) for i in range(min(nR, 4))]  # four worlds, scanned from 16 cycles each
    poses, obs = [], []
    for i in range(nR):
        ins = worlds[i % len(worlds)]
        pts = synth.laser_scan(ins, i // len(worlds), z=0.3, z_jitter=1.5)
        poses.append([float(v) for v in ins["pos"]])
        obs.append(dict(instance=i, points=pts, origin=(poses[-1][0], poses[-1][1], 0.55), obstacle_range=2.5, raytrace_range=3.0))
    fl.stage_observations(poses, obs)
    fl.update_map()
    fl.sync()
    fl.profile_select(["k_voxel_export"])
    fl.profile(True)
    dev, wall, host = [], [], []
    for i in range(args.warmup + args.steps):
        fl.profile_reset()
        t0 = time.perf_counter()
        got = fl.voxel_points(N.VOXEL_MARKED)
        t1 = time.perf_counter()
        ms, launches = fl.profile_read()["k_voxel_export"]
        assert launches == 3  # count + scan of both passes, emit of the second
        if i >= args.warmup:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    fl.profile(False)
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        want = host_marked_points(fl)
        t1 = time.perf_counter()
        if i >= args.warmup:
            host.append((t1 - t0) * 1e3)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), "the two answers differ"
    out = {"robots": nR, "size": n, "z_voxels": Z_VOXELS, "marked_points": int(sum(len(g) for g in got)),
           "timing": f"median of {args.steps} after {args.warmup}; device = HIP events around the launches, wall = the whole call",
           "voxel_points_device_ms": round(float(np.median(dev)), 4), "voxel_points_wall_ms": round(float(np.median(wall)), 4),
           "host_download_classify_wall_ms": round(float(np.median(host)), 4)}
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
