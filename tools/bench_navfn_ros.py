#!/usr/bin/env python3
"""Time NavfnROS::makePlan for 256 plans on 400 x 400 maps (tolerance 0.5 m at 0.05 m) two ways, in alternating blocks in one process:
  (a) navgpu_navfn_ros_make_plan + navgpu_navfn_ros_plans: world poses in, the concatenated world plans out
  (b) the calls there were before: cells made in numpy, navgpu_navfn_plan, one navgpu_navfn_potential read-back per plan, the
      tolerance window in numpy, navgpu_navfn_plan again from the best cells for the second path (there was no other way to walk
      from another cell), one navgpu_navfn_path per plan, then the poses assembled in numpy
Route (b)'s second plan call expands again, until the best cell rather than the goal's has a potential, and walks with
calcPath(nx * ny / 2) where the reference's second walk has nx * 4 steps: its poses are compared with route (a)'s once and the
outcome reported (same_poses), a difference there being route (b)'s.  Also timed: navgpu_navfn_plan alone (the expansion,
which both routes share: what is claimed is the time outside it), navgpu_navfn_ros_plan_from_potential (the second calcPath alone),
navgpu_navfn_ros_valid_point_potential with one point per plan (the window kernel's OR form - no sqrt, no cost - with the
host's sequence build, upload and result copy; the cost form is not timed on its own), and
navgpu_navfn_ros_potential_cloud against 256 potential read-backs + numpy.nonzero and the same arithmetic.
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
    s_map, g_map = rs.uniform(12, n - 13, (n_plans, 2)), rs.uniform(12, n - 13, (n_plans, 2))
    cm = maps[np.arange(n_plans) % n_maps].copy()
    for k in range(n_plans):
        x, y = s_map[k]
        cm[k, int(y) - 1:int(y) + 3, int(x) - 1:int(x) + 3] = 0
        x, y = g_map[k]
        if k % 2:  # every other goal sits in a lethal blob: the window has work to do
            cm[k, int(y) - 2:int(y) + 3, int(x) - 2:int(x) + 3] = 254
        else:
            cm[k, int(y) - 1:int(y) + 3, int(x) - 1:int(x) + 3] = 0
    world = lambda p: frames[:, :2] + (p + 0.5) * frames[:, 2:3]  # noqa: E731
    starts = np.concatenate([world(s_map), rs.uniform(-3, 3, (n_plans, 1))], axis=1)
    goals = np.concatenate([world(g_map), rs.uniform(-3, 3, (n_plans, 1))], axis=1)
    return cm, frames, starts, goals


def sequence(c, tol, res):
    out, p = [], c - tol
    while p <= c + tol:
        out.append(p)
        p += res
    return np.array(out)


def numpy_window(pot, frame, goal, tol, w_dist, w_len):
    """the tolerance search over one potential array -> (x, y, cell) of the best candidate, or None"""
    ny, nx = pot.shape
    ox, oy, res = frame
    xs, ys = sequence(goal[0], tol, res), sequence(goal[1], tol, res)
    px, py = np.meshgrid(xs, ys)
    with np.errstate(invalid="ignore"):
        on = (px >= ox) & (py >= oy)
        cx, cy = ((px - ox) / res).astype(np.int64), ((py - oy) / res).astype(np.int64)
    on &= (cx < nx) & (cy < ny)
    p = np.full(px.shape, np.inf)
    p[on] = pot[cy[on], cx[on]]
    with np.errstate(invalid="ignore"):
        cost = np.sqrt((px - goal[0]) ** 2 + (py - goal[1]) ** 2) * w_dist + p * w_len
    cost[~(p < 1.0e10)] = np.inf
    i = int(np.argmin(cost))  # the first of equal minima in row-major order: the scan order
    if not cost.flat[i] < np.finfo(np.float64).max:
        return None
    return float(px.flat[i]), float(py.flat[i]), (int(cx.flat[i]), int(cy.flat[i]))


def the_old_way(nf, frames, starts, goals, tol, w, t):
    """(b): -> (poses, offsets), the parts' times added to t"""
    n = len(starts)
    t0 = time.perf_counter()
    robot = ((starts[:, :2] - frames[:, :2]) / frames[:, 2:3]).astype(np.int32)
    cells = ((goals[:, :2] - frames[:, :2]) / frames[:, 2:3]).astype(np.int32)
    nf.plan(robot, cells)
    t1 = time.perf_counter()
    pots = [nf.potential(k) for k in range(n)]
    t2 = time.perf_counter()
    best = [numpy_window(pots[k], frames[k], goals[k], tol, *w) for k in range(n)]
    t3 = time.perf_counter()
    have = [k for k in range(n) if best[k] is not None]
    second = np.array([best[k][2] if best[k] else cells[k] for k in range(n)], np.int32)
    res = nf.plan(robot, second)
    t4 = time.perf_counter()
    out, offsets = [], [0]
    for k in range(n):
        m = res[k].path_length if best[k] is not None else 0
        if m:
            xy = np.zeros((m, 2), np.float32)
            nf.L.navgpu_navfn_path(nf.h, k, xy.ctypes.data_as(C.c_void_p), m)
            q = xy[::-1].astype(np.float64)
            poses = np.zeros((m + 1, 3))
            poses[:-1, 0] = frames[k, 0] + q[:, 0] * frames[k, 2]
            poses[:-1, 1] = frames[k, 1] + q[:, 1] * frames[k, 2]
            poses[-1] = (best[k][0], best[k][1], goals[k, 2])
            out.append(poses)
        offsets.append(offsets[-1] + (m + 1 if m else 0))
    poses = np.concatenate(out) if out else np.zeros((0, 3))
    t5 = time.perf_counter()
    t["b_plan"].append(t1 - t0), t["b_potentials"].append(t2 - t1), t["b_window"].append(t3 - t2), t["b_second_plan"].append(t4 - t3)
    t["b_paths_assembly"].append(t5 - t4), t["b_total"].append(t5 - t0), t["b_outside_expansion"].append(t5 - t1)
    return poses, np.array(offsets, np.uint32), len(have)


def the_new_way(nf, frames, starts, goals, tol, w, t):
    t0 = time.perf_counter()
    res = nf.navfn_ros_make_plan(frames, starts, goals, tol, w_dist=w[0], w_len=w[1])
    t1 = time.perf_counter()
    total = sum(r.n_poses for r in res)
    poses, offsets = nf.navfn_ros_plans(0, len(res), capacity=total)
    t2 = time.perf_counter()
    t["a_make_plan"].append(t1 - t0), t["a_plans"].append(t2 - t1), t["a_total"].append(t2 - t0)
    return poses, offsets, res


def numpy_cloud(nf, frames, starts_cells, n):
    out = []
    for k in range(n):
        pot = nf.potential(k)
        flat = pot.reshape(-1)
        keep = np.nonzero(flat.astype(np.float64) < 10e7)[0]
        pts = np.zeros((len(keep), 4), np.float32)
        pts[:, 0] = (frames[k, 0] + (keep % pot.shape[1]).astype(np.float64) * frames[k, 2]).astype(np.float32)
        pts[:, 1] = (frames[k, 1] + (keep // pot.shape[1]).astype(np.float64) * frames[k, 2]).astype(np.float32)
        with np.errstate(all="ignore"):
            pts[:, 2] = flat[keep] / pot[starts_cells[k][1], starts_cells[k][0]] * np.float32(20)
        pts[:, 3] = flat[keep]
        out.append(pts)
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--tolerance", type=float, default=0.5)
    a = ap.parse_args()
    w = (1.0, 0.0)
    cm, frames, starts, goals = make_inputs(a.plans, a.size, a.maps, a.seed)
    nf = nav.NavFn(a.size, a.size, a.plans)
    nf.set_costmap(cm, cost_mode=1)
    keys = ("a_make_plan", "a_plans", "a_total", "b_plan", "b_potentials", "b_window", "b_second_plan", "b_paths_assembly", "b_total",
            "b_outside_expansion")
    warm = {k: [] for k in keys}
    pa, oa, res = the_new_way(nf, frames, starts, goals, a.tolerance, w, warm)
    pb, ob, _ = the_old_way(nf, frames, starts, goals, a.tolerance, w, warm)
    same = bool(np.array_equal(oa, ob) and pa.tobytes() == np.ascontiguousarray(pb).tobytes())
    robot = np.array([r.start_cell[:] for r in res], np.int32)
    cells = np.array([r.goal_cell[:] for r in res], np.int32)
    best_poses = np.array([[r.best_x, r.best_y, 0.0] if r.best_cell[0] >= 0 else list(goals[k]) for k, r in enumerate(res)])
    t = {k: [] for k in keys}
    t.update(expansion_alone=[], a_outside_expansion=[], plan_from_potential=[], valid_point_potential=[], cloud=[], cloud_numpy=[])
    same_cloud = None
    for _ in range(a.blocks):
        the_new_way(nf, frames, starts, goals, a.tolerance, w, t)
        the_old_way(nf, frames, starts, goals, a.tolerance, w, t)
        t0 = time.perf_counter()
        nf.plan(robot, cells)
        t["expansion_alone"].append(time.perf_counter() - t0)
        t["a_outside_expansion"].append(t["a_total"][-1] - t["expansion_alone"][-1])
        res = nf.navfn_ros_make_plan(frames, starts, goals, a.tolerance)
        t0 = time.perf_counter()
        nf.navfn_ros_plan_from_potential(frames, best_poses)
        t1 = time.perf_counter()
        nf.navfn_ros_valid_point_potential(frames, [g[None, :2] for g in goals], a.tolerance)
        t2 = time.perf_counter()
        pts, off = nf.navfn_ros_potential_cloud(frames)  # count-only, then the points: two calls
        t3 = time.perf_counter()
        ref = numpy_cloud(nf, frames, [r.goal_cell[:] for r in res], a.plans)
        t4 = time.perf_counter()
        t["plan_from_potential"].append(t1 - t0), t["valid_point_potential"].append(t2 - t1), t["cloud"].append(t3 - t2), t["cloud_numpy"].append(t4 - t3)
        if same_cloud is None:  # (after plan_from_potential NavFn's start is the cell of the pose it walked from: the goal's where no best)
            same_cloud = bool(int(off[-1]) == len(ref) and pts[:, [0, 1, 3]].tobytes() == ref[:, [0, 1, 3]].tobytes())
    out = dict(tool="bench_navfn_ros", plans=a.plans, size=a.size, blocks=a.blocks, tolerance=a.tolerance, poses=int(oa[-1]),
               plans_found=int((np.diff(oa) > 0).sum()), same_poses=same, same_cloud_xy_pot=same_cloud, cloud_points=int(off[-1]))
    for k, v in t.items():
        ms = np.array(v) * 1e3
        out[k + "_ms"] = dict(median=round(float(np.median(ms)), 3), min=round(float(ms.min()), 3), max=round(float(ms.max()), 3))
    print(json.dumps(out))
    nf.close()


if __name__ == "__main__":
    main()
