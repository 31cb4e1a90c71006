#!/usr/bin/env python3
"""Time navgpu_local_planner_compute_velocity_commands per fleet cycle with the robots' global plans kept two ways, in alternating
blocks in one process and one build:
  (host)     navgpu_local_planner_set_plan: the plan in a host vector; every cycle walks it, repacks the window and uploads it
  (resident) navgpu_local_planner_set_plans: the plan in the device store; every cycle runs k_plan_window and reads 64 B per robot
for 256 robots on empty 400 x 400 maps and plans of 500 and 4000 poses.  A plan is a straight diagonal line of poses 2.5 cm apart
that starts 20 poses behind the robot: the window is the ~420 poses up to the edge of the reach (max_plan 512), a long plan goes
on beyond it.  A third case puts the window deep in a 4000-pose plan with pruning off (3520 poses the robot has left behind, out of
reach, stay in front of it: the host path walks them every cycle).  Both fleets get the same poses every cycle; their results are
compared once, byte for byte.

Then the hand-over of a NavFn batch's plans: navgpu_local_planner_adopt_plans against navgpu_global_planner_plans (the read-back)
plus one navgpu_local_planner_set_plan per robot.

Times are host wall clock around calls that end in a stream synchronise (the control cycle reads its results at its end; an
adoption is followed by navgpu_sync).  Prints one JSON line: medians and (min, max) in ms; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402
from navigation_amd import _lib as N  # noqa: E402

RES = 0.05


def make_fleet(n_robots, n, max_plan, prune):
    cfg = nav.DwaConfig(vx_samples=8, vy_samples=3, vth_samples=9, sim_time=1.2, sim_granularity=0.1, discretize_by_time=1)
    fl = nav.Fleet(n_robots, n, n, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=32, max_plan=max_plan)
    fl.configure_planner(cfg)
    fl.set_footprint(np.array([[0.2, 0.2], [0.2, -0.2], [-0.2, -0.2], [-0.2, 0.2]]))
    fl.configure_local_planner(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, rot_stopped_vel=0.01, trans_stopped_vel=0.01,
                               max_rot_vel=cfg.max_rot_vel, min_rot_vel=cfg.min_rot_vel, acc_lim_x=cfg.acc_lim_x, acc_lim_y=cfg.acc_lim_y,
                               acc_lim_theta=cfg.acc_lim_theta, sim_period=cfg.sim_period, prune_plan=int(prune), latch_xy_goal_tolerance=0)
    return fl


def line_plan(centre, n_poses, behind, k):
    """poses 2.5 cm apart on a diagonal through the robot that starts 20 poses behind it; the `behind - 20` poses before those lie out
    of reach, 100 m away (a part of the plan the robot has long left, kept because pruning is off); robot k's line is shifted a little"""
    a = np.pi / 4 + 0.002 * (k % 11)
    d = np.cos(a), np.sin(a)
    s = (np.arange(n_poses) - behind) * 0.025
    x, y = centre + s * d[0], centre + 0.01 * (k % 7) + s * d[1]
    x[:max(behind - 20, 0)] += 100.0
    return np.stack([x, y, np.full(n_poses, a)], 1)


def stats(ms):
    ms = np.asarray(ms)
    return dict(median=round(float(np.median(ms)), 4), min=round(float(ms.min()), 4), max=round(float(ms.max()), 4), n=int(len(ms)))


def time_cycles(fleets, poses, vels, blocks, per_block, warmup):
    """alternating blocks of cycles on each fleet -> {name: [ms per cycle]}; the poses are the same every cycle"""
    arr = {name: fl._robot_inputs(poses, vels, None) for name, fl in fleets.items()}
    out = {name: (N.CmdResult * len(poses))() for name in fleets}
    ms = {name: [] for name in fleets}

    def cycle(name):
        fl = fleets[name]
        t0 = time.perf_counter()
        rc = fl.L.navgpu_local_planner_compute_velocity_commands(fl.h, 0, len(poses), arr[name], out[name])
        t1 = time.perf_counter()
        assert rc == 0, (name, rc, fl.L.navgpu_last_error())
        return (t1 - t0) * 1e3

    for name in fleets:
        for _ in range(warmup):
            cycle(name)
    for _ in range(blocks):
        for name in fleets:
            ms[name] += [cycle(name) for _ in range(per_block)]
    same = len({bytes(o) for o in out.values()}) == 1
    n_ok = sum(int(r.ok) for r in out["resident"])
    n_dwa = sum(int(r.branch == N.BRANCH_DWA) for r in out["resident"])
    return ms, same, n_ok, n_dwa, int(out["resident"][0].local_plan_points)


def bench_cycles(a, n_poses, behind, prune):
    centre = a.cells * RES / 2
    plans = [line_plan(centre, n_poses, behind, k) for k in range(a.robots)]
    fleets = dict(host=make_fleet(a.robots, a.cells, a.max_plan, prune), resident=make_fleet(a.robots, a.cells, a.max_plan, prune))
    fleets["resident"].reserve_global_plans(max(n_poses, 16))
    for k, p in enumerate(plans):
        fleets["host"].set_global_plan(k, p)
    fleets["resident"].set_global_plans(plans)
    poses = np.array([[centre, centre + 0.01 * (k % 7), np.pi / 4] for k in range(a.robots)])
    vels = np.tile([0.2, 0.0, 0.0], (a.robots, 1))
    ms, same, n_ok, n_dwa, n_local = time_cycles(fleets, poses, vels, a.blocks, a.per_block, a.warmup)
    w = fleets["resident"].local_windows()[0]
    for fl in fleets.values():
        fl.close()
    return dict(plan_poses=n_poses, first_pose_behind=behind, prune=int(prune), window_first_index=int(w.first_index), local_plan_points=n_local,
                robots_ok=n_ok, robots_on_dwa=n_dwa, results_byte_equal=bool(same), host_ms=stats(ms["host"]), resident_ms=stats(ms["resident"]))


def bench_adoption(a):
    """256 plans of a NavFn batch over the fleet's (empty) master grids -> adopted on the device / read back and set per robot"""
    n, size = a.robots, a.cells * RES
    res_fl, host_fl = make_fleet(n, a.cells, a.max_plan, 1), make_fleet(n, a.cells, a.max_plan, 1)
    res_fl.reserve_global_plans(4 * a.cells)  # calcPath allows 4 * nx
    nf = nav.NavFn(a.cells, a.cells, n)
    nf.set_costmap_from_fleet(res_fl)
    rs = np.random.RandomState(3)
    starts = np.concatenate([rs.uniform(0.1 * size, 0.3 * size, (n, 2)), rs.uniform(-3, 3, (n, 1))], 1)
    goals = np.concatenate([rs.uniform(0.7 * size, 0.9 * size, (n, 2)), rs.uniform(-3, 3, (n, 1))], 1)
    made = nf.make_plan((0.0, 0.0, RES), starts, goals, orientation_mode=1, wavefront=True)
    lengths = [r.n_poses for r in made]
    t_adopt, t_back = [], []
    for it in range(a.warmup + a.adopt_reps):
        t0 = time.perf_counter()
        adopted = res_fl.adopt_global_plans(nf, N.PLAN_FAMILY_GLOBAL_PLANNER)
        res_fl.sync()
        t1 = time.perf_counter()
        poses, off = nf.plans()
        for k in range(n):
            host_fl.set_global_plan(k, poses[off[k]:off[k + 1]])
        host_fl.sync()
        t2 = time.perf_counter()
        if it >= a.warmup:
            t_adopt.append((t1 - t0) * 1e3)
            t_back.append((t2 - t1) * 1e3)
    same = all(res_fl.global_plan(k).tobytes() == host_fl.global_plan(k).tobytes() for k in (0, n // 2, n - 1))
    nf.close()
    res_fl.close()
    host_fl.close()
    return dict(plans=n, adopted=int(sum(adopted)), poses_min=int(min(lengths)), poses_max=int(max(lengths)), plans_byte_equal=bool(same),
                adopt_ms=stats(t_adopt), readback_set_plan_ms=stats(t_back))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--robots", type=int, default=256)
    p.add_argument("--cells", type=int, default=400)
    p.add_argument("--max-plan", type=int, default=512)
    p.add_argument("--plan-poses", type=int, nargs="+", default=[500, 4000])
    p.add_argument("--blocks", type=int, default=6)
    p.add_argument("--per-block", type=int, default=25)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--adopt-reps", type=int, default=10)
    p.add_argument("--no-adoption", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if nav.lib().navgpu_device_count() <= 0:
        sys.exit("bench_local_plan: needs a GPU (there is no other way to take these times)")
    cycles = []
    for n_poses in a.plan_poses:
        cycles.append(bench_cycles(a, n_poses, behind=20, prune=1))  # the robot near the front of its stored plan: what pruning keeps true
    # the window deep in the stored plan (pruning off, as a caller that wants the whole plan kept would run it)
    deep = max(a.plan_poses) - 460
    if deep > 0:
        cycles.append(bench_cycles(a, max(a.plan_poses), behind=deep, prune=0))
    result = dict(tool="bench_local_plan", robots=a.robots, cells=a.cells, max_plan=a.max_plan, cycles_per_path=a.blocks * a.per_block,
                  timing="host wall clock, ms per fleet cycle; each call ends in a stream synchronise", cycles=cycles)
    if not a.no_adoption:
        result["adoption"] = bench_adoption(a)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
