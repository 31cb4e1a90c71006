#!/usr/bin/env python3
"""Time GlobalPlanner::makePlan for 256 plans on 400 x 400 maps two ways, in alternating blocks in one process:
  (a) navgpu_global_planner_make_plan + navgpu_global_planner_plans: world poses in, the concatenated world plans out
  (b) the calls there were before: map coordinates made in numpy, navgpu_global_planner_plan, one navgpu_navfn_path per plan,
      then the same poses assembled in numpy (reverse, mapToWorld, goal, forward orientations)
and navgpu_global_planner_potential_grid for the 256 plans against 256 navgpu_navfn_potential read-backs.  Orientation mode
FORWARD (GlobalPlanner.cfg's default; it vectorises in numpy, so (b) is not charged a Python loop).  Both ways see the same cost
bytes (the start cells are cleared before the upload) and their poses are compared once: positions bit for bit, yaws to 1e-12.
Times are host wall clock around calls that end in a stream synchronise.  Prints one JSON line: medians and (min, max) in ms."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402


def make_inputs(n_plans, n, n_maps, seed):
    rs = np.random.RandomState(seed)
    maps = np.zeros((n_maps, n, n), np.uint8)
    for m in maps:
        m[rs.random_sample((n, n)) < 0.03] = 254
        blur = (rs.random_sample((n, n)) < 0.15) & (m == 0)
        m[blur] = rs.randint(1, 253, blur.sum())
    frames = np.stack([rs.uniform(-3, 3, n_plans), rs.uniform(-3, 3, n_plans), np.full(n_plans, 0.05)], axis=1)
    s_map, g_map = rs.uniform(8, n - 9, (n_plans, 2)), rs.uniform(8, n - 9, (n_plans, 2))
    cm = maps[np.arange(n_plans) % n_maps].copy()
    for k in range(n_plans):
        for x, y in (s_map[k], g_map[k]):
            cm[k, int(y) - 1:int(y) + 3, int(x) - 1:int(x) + 3] = 0
    world = lambda p: frames[:, :2] + (p + 0.5) * frames[:, 2:3]  # noqa: E731
    starts = np.concatenate([world(s_map), rs.uniform(-3, 3, (n_plans, 1))], axis=1)
    goals = np.concatenate([world(g_map), rs.uniform(-3, 3, (n_plans, 1))], axis=1)
    return cm, frames, starts, goals


def the_old_way(nf, frames, starts, goals, t):
    """(b): -> (poses, offsets), the parts' times added to t"""
    t0 = time.perf_counter()
    s = (starts[:, :2] - frames[:, :2]) / frames[:, 2:3] - 0.5
    g = (goals[:, :2] - frames[:, :2]) / frames[:, 2:3] - 0.5
    cells = ((goals[:, :2] - frames[:, :2]) / frames[:, 2:3]).astype(np.int32)
    res = nf.global_planner_plan(s, g, cells)
    t1 = time.perf_counter()
    paths = []
    for k, r in enumerate(res):
        xy = np.zeros((max(r.path_length, 1), 2), np.float32)
        nf.L.navgpu_navfn_path(nf.h, k, xy.ctypes.data_as(C.c_void_p), r.path_length)
        paths.append(xy[:r.path_length])
    t2 = time.perf_counter()
    out, offsets = [], [0]
    for k, p in enumerate(paths):
        if len(p):
            q = p[::-1].astype(np.float64)
            poses = np.empty((len(q) + 1, 3))
            poses[:-1, 0] = frames[k, 0] + (q[:, 0] + 0.5) * frames[k, 2]
            poses[:-1, 1] = frames[k, 1] + (q[:, 1] + 0.5) * frames[k, 2]
            poses[-1] = goals[k]
            poses[:-1, 2] = np.arctan2(np.diff(poses[:, 1]), np.diff(poses[:, 0]))
            out.append(poses)
        offsets.append(offsets[-1] + (len(p) + 1 if len(p) else 0))
    poses = np.concatenate(out) if out else np.zeros((0, 3))
    t3 = time.perf_counter()
    t["b_plan"].append(t1 - t0), t["b_paths"].append(t2 - t1), t["b_assembly"].append(t3 - t2), t["b_total"].append(t3 - t0)
    return poses, np.array(offsets, np.uint32)


def the_new_way(nf, frames, starts, goals, t):
    t0 = time.perf_counter()
    res = nf.make_plan(frames, starts, goals, orientation_mode=1)
    t1 = time.perf_counter()
    total = sum(r.n_poses for r in res)
    poses, offsets = nf.plans(0, len(res), capacity=total)
    t2 = time.perf_counter()
    t["a_make_plan"].append(t1 - t0), t["a_plans"].append(t2 - t1), t["a_total"].append(t2 - t0)
    return poses, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    cm, frames, starts, goals = make_inputs(a.plans, a.size, a.maps, a.seed)
    sc = ((starts[:, :2] - frames[:, :2]) / frames[:, 2:3]).astype(int)
    cm[np.arange(a.plans), sc[:, 1], sc[:, 0]] = 0  # clearRobotCell, done by hand for (b)
    nf = nav.NavFn(a.size, a.size, a.plans)
    nf.set_costmap(cm, cost_mode=0)
    warm = {k: [] for k in ("a_make_plan", "a_plans", "a_total", "b_plan", "b_paths", "b_assembly", "b_total")}
    pa, oa = the_new_way(nf, frames, starts, goals, warm)
    pb, ob = the_old_way(nf, frames, starts, goals, warm)
    same = bool(np.array_equal(oa, ob) and np.array_equal(pa[:, :2].view(np.uint64), np.ascontiguousarray(pb[:, :2]).view(np.uint64)) and
                (len(pa) == 0 or float(np.abs(pa[:, 2] - pb[:, 2]).max()) <= 1e-12))
    t = {k: [] for k in warm}
    t.update(grid=[], potential_readbacks=[])
    for _ in range(a.blocks):
        the_new_way(nf, frames, starts, goals, t)
        the_old_way(nf, frames, starts, goals, t)
        t0 = time.perf_counter()
        nf.potential_grid(0, a.plans)
        t1 = time.perf_counter()
        for k in range(a.plans):
            nf.potential(k)
        t["grid"].append(t1 - t0), t["potential_readbacks"].append(time.perf_counter() - t1)
    out = dict(tool="bench_global_plan", plans=a.plans, size=a.size, blocks=a.blocks, poses=int(oa[-1]), plans_found=int((np.diff(oa) > 0).sum()),
               same_poses=same)
    for k, v in t.items():
        ms = np.array(v) * 1e3
        out[k + "_ms"] = dict(median=round(float(np.median(ms)), 3), min=round(float(ms.min()), 3), max=round(float(ms.max()), 3))
    print(json.dumps(out))
    nf.close()


if __name__ == "__main__":
    main()
