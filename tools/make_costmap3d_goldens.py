#!/usr/bin/env python3
"""Writes tests/golden/costmap3d/c3d_reference.npz: 48 poses of the test robot on the aisles map and the yardstick's answers.

  python3 tools/make_costmap3d_goldens.py

40 poses are (x, y, yaw) uniform over the map at z = 0, 8 more carry a roll or a pitch of +-0.1 rad.  The answers are those of
tests/costmap3d_ref.py (numpy, float64) in distance mode without a limit: -1.0 for a collision, else the distance.  A pose is
decided when the yardstick's verdict is the same with the cells' half edges scaled by 1 - 1e-6, 1 and 1 + 1e-6 and, when free,
its distance exceeds 1e-6; the seed is the first one for which every pose is decided, so the file holds no borderline case.
Needs no GPU and nothing of the library but its two file readers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import costmap3d_ref as ref  # noqa: E402
from navigation_amd.costmap3d import load_stl, read_octomap_bt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")
SCALES = (1.0 - 1e-6, 1.0, 1.0 + 1e-6)


def aisles():
    """the map as the tests place it: (origin, size_xyz, resolution, cells (N, 3), tree)"""
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    lo = (t["centres"] - 0.5 * t["sizes"][:, None]).min(0)
    hi = (t["centres"] + 0.5 * t["sizes"][:, None]).max(0)
    cells = ref.boxes_to_cells(t["centres"], t["sizes"], lo, t["res"])
    return lo, np.rint((hi - lo) / t["res"]).astype(int), t["res"], cells, t


def rpy_quaternion(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def poses_of(seed, lo, hi):
    rng = np.random.default_rng(seed)
    poses = []
    for k in range(48):
        x, y, yaw = rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), rng.uniform(-np.pi, np.pi)
        tilt = (0.0, 0.0) if k < 40 else [(0.1, 0.0), (-0.1, 0.0), (0.0, 0.1), (0.0, -0.1)][k % 4]
        poses.append([x, y, 0.0] + rpy_quaternion(tilt[0], tilt[1], yaw))
    return np.array(poses)


def answers(poses, centres, res, vertices, triangles):
    verdict = np.zeros((len(SCALES), len(poses)), bool)
    cost = np.zeros(len(poses))
    for k, p in enumerate(poses):
        for s, scale in enumerate(SCALES):
            c = ref.query_pose(centres, res, vertices, triangles, p, mode=ref.DISTANCE if scale == 1.0 else ref.COLLISION_ONLY, closed=True,
                               half_scale=scale)
            verdict[s, k] = c < 0.0
            if scale == 1.0:
                cost[k] = c
    decided = (verdict == verdict[1]).all(0) & (verdict[1] | (cost > 1e-6))
    return cost, verdict, decided


def main():
    origin, size, res, cells, _ = aisles()
    centres = ref.cell_centres(cells, origin, res)
    vertices, triangles = load_stl(os.path.join(GOLDEN, "test_robot.stl"))
    assert ref.mesh_closed(triangles)
    for seed in range(100):
        poses = poses_of(seed, origin, origin + size * res)
        cost, verdict, decided = answers(poses, centres, res, vertices, triangles)
        print(f"seed {seed}: {int(verdict[1].sum())} collide, {int((~verdict[1]).sum())} free, {int((~decided).sum())} undecided, "
              f"free distances {cost[cost >= 0].min():.6f} .. {cost[cost >= 0].max():.6f}")
        if decided.all():
            break
    else:
        raise SystemExit("no seed below 100 leaves every pose decided")
    np.savez(os.path.join(GOLDEN, "c3d_reference.npz"), seed=seed, poses=poses, cost=cost, verdict=verdict, decided=decided)


if __name__ == "__main__":
    main()
