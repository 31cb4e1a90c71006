#!/usr/bin/env python3
"""Time move_base's executive calls against the routes a build without them forces, on one GPU:
  handover  navgpu_move_base_handover_plans for --robots robots whose controller plans and new plans have about 1000 poses, half of
            them adopting, against: read the new plans back (navgpu_*_plans), read every controller plan back
            (navgpu_local_planner_get_plan), MoveBase::preferPrevPlan in numpy, navgpu_local_planner_set_plans for the adopters
  polygon   navgpu_move_base_clear_costmap_windows (a 3 m x 3 m window) on --robots x 400 x 400 master grids, against:
            navgpu_grid_download, a numpy fill of the same cells, navgpu_grid_upload
  service   navgpu_move_base_plan_service for one request of 49 candidates on the reference's willow_costmap (1132 x 1217; navfn_ros
            family, the bit-exact expansion): the goal is a lethal cell whose first reachable candidate is the first of ring 2, so the
            winner is candidate 9.  One round on 49 slots against the same candidates as single-slot navgpu_navfn_ros_make_plan calls one
            after the other on the same build, stopping at the first success as the reference does; with the time of one single call
            what one round costs in single calls (the crossover) and the slots' memory follow
Wall time of the whole call or route on the host (every call here returns synchronised), after --warmup runs, median and spread of
--steps runs.  Clocks are left as the machine has them.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import navigation_amd as nav  # noqa: E402
from navigation_amd import _lib as N, synth  # noqa: E402
import move_base_ref as R  # noqa: E402

NOW, TIMEOUT = 50_000_000_000, 10_000_000_000


def stats(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=round(float(np.median(a)), 4), min_ms=round(float(a[0]), 4), max_ms=round(float(a[-1]), 4), runs=len(a))


def timed(fn, steps, warmup, before=None):
    out = []
    for i in range(warmup + steps):
        if before:
            before()
        t = time.perf_counter()
        fn()
        if i >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def walls(n):
    m = np.zeros((n, n), np.uint8)
    m[n // 3, :n - 20] = 254
    m[2 * n // 3, 20:] = 254
    return m


def bench_handover(robots, steps, warmup):
    n = 200
    cfg = nav.DwaConfig(vx_samples=6, vy_samples=1, vth_samples=7, sim_time=1.0, sim_granularity=0.1, discretize_by_time=1)
    fl = nav.Fleet(robots, n, n, synth.RES, layers=N.LAYER_OBSTACLE, max_sim_steps=32, max_plan=512)
    fl.configure_planner(cfg)
    fl.set_footprint(synth.FOOTPRINT)
    fl.upload(N.GRID_MASTER, np.broadcast_to(walls(n), (robots, n, n)))
    fl.configure_local_planner(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, rot_stopped_vel=0.01, trans_stopped_vel=0.01,
                               max_rot_vel=cfg.max_rot_vel, min_rot_vel=cfg.min_rot_vel, acc_lim_x=cfg.acc_lim_x, acc_lim_y=cfg.acc_lim_y,
                               acc_lim_theta=cfg.acc_lim_theta, sim_period=cfg.sim_period, prune_plan=1, latch_xy_goal_tolerance=0)
    fl.reserve_global_plans(2048)
    nf = nav.NavFn(n, n, robots)
    nf.set_costmap(walls(n), cost_mode=0)
    res = nf.make_plan((0.0, 0.0, synth.RES), np.tile((0.525, 0.525, 0.3), (robots, 1)), np.tile((9.475, 9.475, 1.0), (robots, 1)),
                       orientation_mode=1)
    new_len = res[0].n_poses
    assert all(r.n_poses == new_len for r in res) and new_len > 400
    # controller plans of about 1000 poses; the robot stands near pose 900, so prev_len is about 100 and the new plan is much longer
    i = np.arange(1000)
    controller = np.stack([1.0 + 0.008 * i, np.full(1000, 1.0), np.zeros(1000)], 1)
    pos = np.tile((1.0 + 0.008 * 900, 1.0), (robots, 1))
    states = np.where(np.arange(robots) % 2 == 0, R.PERSISTENCE_INITIAL, NOW + 5).astype(np.int64)  # even robots adopt, odd ones keep

    def reset():
        fl.set_global_plans([controller] * robots)
        fl.set_plan_persistence(states)

    def new_call():
        fl.handover_global_plans(nf, N.PLAN_FAMILY_GLOBAL_PLANNER, pos, NOW, TIMEOUT)

    host_states = states.copy()

    def parent_route():
        poses, off = nf.plans()
        adopt, plans = [], []
        for k in range(robots):
            cp = fl.global_plan(k)
            ci = R.find_closest_plan_index(cp[:, :2], pos[k])
            keep, host_states[k] = R.prefer_prev_plan(int(states[k]), len(cp), ci, int(off[k + 1] - off[k]), NOW, TIMEOUT)
            if not keep:
                adopt.append(k)
                plans.append(poses[off[k]:off[k + 1]])
        for k, p in zip(adopt, plans):  # (runs of adopters; here every other robot)
            fl.set_global_plans([p], first=k)

    reset()
    rec = fl.handover_global_plans(nf, N.PLAN_FAMILY_GLOBAL_PLANNER, pos, NOW, TIMEOUT)
    decisions = [r.decision for r in rec]
    out = dict(robots=robots, decisions_as_planned=decisions == [N.HANDOVER_ADOPT, N.HANDOVER_KEEP] * (robots // 2), new_len=int(new_len), controller_len=1000, adopting=decisions.count(N.HANDOVER_ADOPT),
               handover_call=timed(new_call, steps, warmup, reset), readback_route=timed(parent_route, steps, warmup, reset))
    nf.close()
    fl.close()
    return out


def bench_polygon(robots, steps, warmup):
    n = 400
    fl = nav.Fleet(robots, n, n, synth.RES, layers=N.LAYER_OBSTACLE)
    start = np.random.RandomState(1).randint(0, 255, (robots, n, n)).astype(np.uint8)
    poses = np.tile((10.0, 10.0), (robots, 1)) + np.random.RandomState(2).uniform(-3, 3, (robots, 2))
    size = 3.0

    def reset():
        fl.upload(N.GRID_MASTER, start)

    def new_call():
        fl.clear_costmap_windows(poses, size, size)

    def parent_route():
        g = fl.master()
        for k, (x, y) in enumerate(poses):  # the same cells: worldToMap of the corners, every cell between them
            x0, x1 = int((x - size / 2) / synth.RES), int((x + size / 2) / synth.RES)
            y0, y1 = int((y - size / 2) / synth.RES), int((y + size / 2) / synth.RES)
            g[k, y0:y1 + 1, x0:x1 + 1] = 0
        fl.upload(N.GRID_MASTER, g)
        return g

    reset()
    new_call()
    a = fl.master()
    reset()
    out = dict(robots=robots, routes_clear_the_same_cells=bool(np.array_equal(a, parent_route())), cells=n, window_m=size, clear_call=timed(new_call, steps, warmup, reset),
               download_fill_upload_route=timed(parent_route, steps, warmup, reset))
    fl.close()
    return out


def bench_service(steps, warmup):
    import gzip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = gzip.open(os.path.join(root, "tests", "golden", "willow_costmap.pgm.gz")).read()
    _, w, h, _, data = raw.split(b"\n", 4)
    nx, ny = int(w), int(h)
    costs = np.frombuffer(data, np.uint8)[:nx * ny].reshape(ny, nx).copy()  # costarr values as they are (cost_mode 0)
    res = 0.05
    frame = (0.0, 0.0, res)
    start = ((428 + 0.5) * res, (746 + 0.5) * res, 0.0)
    goal = ((323 + 0.5) * res, (500 + 0.5) * res, 0.5)
    req = dict(start=start, goal=goal, frame=frame, tolerance=0.5, default_tolerance=0.0)
    cands = R.plan_service_candidates(goal[:2], res, 0.5)
    batch, one = nav.NavFn(nx, ny, len(cands)), nav.NavFn(nx, ny, 1)
    batch.set_costmap(costs, cost_mode=0)
    one.set_costmap(costs, cost_mode=0)
    found = {}

    def one_round():
        found["batch"] = batch.plan_service(N.PLAN_FAMILY_NAVFN_ROS, [req], len(cands))[0][0]

    def single(c):
        return one.navfn_ros_make_plan(frame, [start], [(c[0], c[1], goal[2])], tolerances=0.0)[0]

    def sequential():
        for i, c in enumerate(cands):
            r = single(c)
            if r.status == N.MAKE_PLAN_OK and r.n_poses > 0:
                found["sequential"] = i
                return

    out = dict(map=[nx, ny], candidates=len(cands), one_round=timed(one_round, steps, warmup), sequential_to_first_success=timed(sequential, steps, warmup),
               single_failing_call=timed(lambda: single(cands[0]), steps, warmup))
    w = found["batch"]
    out.update(winner=w.winner, winner_sequential=found["sequential"], n_poses=w.n_poses,
               single_winning_call=timed(lambda: single(cands[w.winner]), steps, warmup))
    # what one round costs in sequential calls: a failing call expands the whole reachable map, a winning one stops at the robot
    out["round_over_failing_call"] = round(out["one_round"]["median_ms"] / out["single_failing_call"]["median_ms"], 2)
    out["round_over_winning_call"] = round(out["one_round"]["median_ms"] / out["single_winning_call"]["median_ms"], 2)
    cells_padded = (nx * ny + 255) // 256 * 256
    out["slot_bytes"] = cells_padded * (1 + 1 + 4 + 4 + 4)  # costarr, pending, potarr, gradx, grady
    out["slots_bytes_total"] = out["slot_bytes"] * len(cands)
    batch.close()
    one.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["handover", "polygon", "service"])
    a = ap.parse_args()
    out = {}
    if a.only in (None, "handover"):
        out["handover"] = bench_handover(a.robots, a.steps, a.warmup)
    if a.only in (None, "polygon"):
        out["polygon"] = bench_polygon(a.robots, a.steps, a.warmup)
    if a.only in (None, "service"):
        out["service"] = bench_service(min(a.steps, 5), min(a.warmup, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
