#!/usr/bin/env python3
"""Time the legacy planner's fleet entry points for 256 robots on the corridor map of tests/golden/g16_tp_reference.npz tiled to 400 x 400
cells, against the same work done through the single entry points.

  probes  256 probes, one per robot, in one navgpu_tp_score_trajectories call            | 256 navgpu_tp_score_trajectory calls
  plans   navgpu_tp_update_plans for 256 robots with compute_dists                        | 256 navgpu_tp_update_plan calls
  stop    navgpu_tp_ros_compute_velocity_commands, every robot on the stop branch         | by hand: window and navgpu_tp_update_plan per robot,
  drive   the same, every robot driving                                                   |   one navgpu_tp_find_best_path, a score call per stopping robot
  mixed   the same call with no robot, every third and every second robot at its goal     | (none: compare with the commit before the listed calls)

The right-hand column uses nothing but entry points the commit before this feature has: run the tool from a checkout of that commit as well
(copy this file into its tools/; the left-hand legs are skipped there) and set the two JSON lines side by side - that is the yardstick, the
same column from this build is only its cross-check.  The answers of the two columns are compared (probes: doubles equal).
Wall time of the whole call (every call ends with a stream wait), median of --steps repetitions after --warmup.

  --ab    the probes leg of the shipped library and of libnavgpu_lpp.so (make -C navigation_amd/csrc tp-probe-ab: one lane per probe)
k_tp_probe alone: run `rocprofv3 --kernel-trace --stats -- python3 tools/bench_tp_ros.py --legs probes` (no counters in that run)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from navigation_amd import _lib as N  # noqa: E402

RES, TILE = 0.05, 64
FP4 = [[0.15, 0.15], [0.15, -0.15], [-0.15, -0.15], [-0.15, 0.15]]


def median_ms(call, steps, warmup):
    t = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return round(float(np.median(t)), 4)


def build(nav, n, size):
    """n robots in the open bands between the tiles' corridors, heading east, each with a 4 m plan straight ahead"""
    import tp_reference_cases as T
    g, meta = T.load()
    tile = T.case(g, meta, "strafe_up_down_up")[1]
    reps = (size + TILE - 1) // TILE
    cells = np.ascontiguousarray(np.tile(tile, (reps, reps))[:size, :size])
    fl = nav.Fleet(n, size, size, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=96, max_plan=256)
    fl.set_origin(np.zeros((n, 2)))
    fl.upload(N.GRID_MASTER, np.broadcast_to(cells, (n, size, size)).copy())
    fl.set_footprint(np.asarray(FP4, np.float64))
    fl.configure_trajectory_planner(N.TpConfig())
    bands = max(1, reps - 2)
    poses = np.array([(2.0 + 0.25 * (k % 37), 3.25 + 3.2 * (k % bands), 0.0) for k in range(n)])
    s = np.arange(0.0, 4.0001, 0.05)
    plans = [np.column_stack([p[0] + s, np.full_like(s, p[1]), np.zeros_like(s)]) for p in poses]
    return fl, poses, plans


def leg_probes(fl, poses, plans, args, out):
    n = len(poses)
    for i, p in enumerate(plans):
        fl.tp_update_plan(i, p[:, :2], compute_dists=True)
    vel, sample = (0.3, 0.0, 0.0), (0.5, 0.0, 0.1)
    probes = np.array([[*poses[i], *vel, *sample] for i in range(n)])

    def loop():
        loop.costs = np.array([fl.tp_score_trajectory(i, probes[i, 0:3], probes[i, 3:6], probes[i, 6:9]) for i in range(n)])
    out["probes"] = {"probes": n, "single_call_loop_wall_ms": median_ms(loop, args.steps, args.warmup)}
    if hasattr(fl, "tp_score_trajectories"):
        inst, off = np.arange(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint32)

        def batched():
            batched.costs = fl.tp_score_trajectories(inst, probes, offsets=off)[0]
        out["probes"]["batched_wall_ms"] = median_ms(batched, args.steps, args.warmup)
        out["probes"]["answers_differ"] = int((batched.costs != loop.costs).sum())
        out["probes"]["legal"] = int((batched.costs >= 0).sum())


def leg_plans(fl, poses, plans, args, out):
    xy = [p[:, :2] for p in plans]

    def loop():
        for i, p in enumerate(xy):
            fl.tp_update_plan(i, p, compute_dists=True)
    out["plans"] = {"robots": len(xy), "single_call_loop_wall_ms": median_ms(loop, args.steps, args.warmup)}
    if hasattr(fl, "tp_update_plans"):
        want = [fl.download(g) for g in (N.GRID_PATH, N.GRID_GOAL)]
        out["plans"]["batched_wall_ms"] = median_ms(lambda: fl.tp_update_plans(xy, compute_dists=True), args.steps, args.warmup)
        out["plans"]["grids_differ"] = int(sum(int(not np.array_equal(fl.download(g), w)) for g, w in zip((N.GRID_PATH, N.GRID_GOAL), want)))


def stop_candidate(cfg, v):
    """stopWithAccLimits (trajectory_planner_ros.cpp:283-290)"""
    sign = lambda x: -1.0 if x < 0.0 else 1.0  # noqa: E731
    return tuple(sign(v[a]) * max(0.0, abs(v[a]) - acc * cfg.sim_period) for a, acc in enumerate((cfg.acc_lim_x, cfg.acc_lim_y, cfg.acc_lim_theta)))


def leg_cycle(fl, poses, plans, stop, args, out):
    """every robot on the stop branch (a plan that ends where it stands, the goal heading 1 rad off, still moving) or every robot driving"""
    n, L = len(poses), N.lib()
    cfg = N.TpConfig()
    vels = np.tile((0.3, 0.0, 0.1), (n, 1))
    if stop:
        s = np.arange(-1.0, 0.0001, 0.05)
        plans = [np.column_stack([p[0] + s, np.full_like(s, p[1]), np.full_like(s, 1.0)]) for p in poses]
    thr = max(fl.nx, fl.ny) * RES / 2.0
    window_out = np.zeros((256, 3))
    pos32, vel32 = poses.astype(np.float32), vels.astype(np.float32)

    def by_hand():
        n_out, n_er = C.c_uint32(), C.c_uint32()
        cmds = []
        for i in range(n):
            p = plans[i]
            L.navgpu_local_plan_window(p.ctypes.data_as(C.c_void_p), len(p), poses[i].ctypes.data_as(C.c_void_p), None, thr, 0,
                                       window_out.ctypes.data_as(C.c_void_p), 256, C.byref(n_out), C.byref(n_er))
            fl.tp_update_plan(i, window_out[:n_out.value, :2], compute_dists=False)
        res = fl.tp_find_best_path(pos32, vel32)
        for i in range(n):
            if stop:
                cand = stop_candidate(cfg, vels[i])
                cmds.append(cand if fl.tp_score_trajectory(i, poses[i], vels[i], cand) >= 0 else (0.0, 0.0, 0.0))
            else:
                cmds.append(tuple(res[i].drive))
        by_hand.cmds = cmds
    key = "stop" if stop else "drive"
    plans = [np.ascontiguousarray(p) for p in plans]
    out[key] = {"robots": n, "by_hand_wall_ms": median_ms(by_hand, args.steps, args.warmup)}
    if hasattr(fl, "tp_ros_compute_velocity_commands"):
        fl.configure_tp_ros(prune_plan=0)
        fl.tp_ros_set_plans(plans)

        def cycle():
            cycle.got = fl.tp_ros_compute_velocity_commands(poses, vels)
        out[key]["fleet_call_wall_ms"] = median_ms(cycle, args.steps, args.warmup)
        want = N.BRANCH_STOP if stop else N.BRANCH_ROLLOUT
        out[key]["on_branch"] = int(sum(g.branch == want and g.ok == 1 for g in cycle.got))
        by_hand()
        out[key]["commands_differ"] = int(sum(tuple(g.cmd_vel) != tuple(c) for g, c in zip(cycle.got, by_hand.cmds)))


def leg_mixed(fl, poses, plans, args, out):
    """navgpu_tp_ros_compute_velocity_commands with some robots at their goal (a plan that ends where they stand, heading as they do) and
    the others driving: none (one contiguous run of driving robots), every third, every second (as many runs as there are driving
    robots).  The commit before the listed calls ran updatePlan + findBestPath once per run."""
    n = len(poses)
    vels = np.tile((0.3, 0.0, 0.1), (n, 1))
    s = np.arange(-1.0, 0.0001, 0.05)
    at_goal = [np.ascontiguousarray(np.column_stack([p[0] + s, np.full_like(s, p[1]), np.zeros_like(s)])) for p in poses]
    drive = [np.ascontiguousarray(p) for p in plans]
    fl.configure_tp_ros(prune_plan=0)
    out["mixed"] = {"robots": n}
    for key, stands in (("goal_0", lambda k: False), ("goal_third", lambda k: k % 3 == 2), ("goal_alternating", lambda k: k % 2 == 1)):
        fl.tp_ros_set_plans([at_goal[k] if stands(k) else drive[k] for k in range(n)])

        def cycle():
            cycle.got = fl.tp_ros_compute_velocity_commands(poses, vels)
        ms = median_ms(cycle, args.steps, args.warmup)
        runs = sum(1 for k in range(n) if not stands(k) and (k == 0 or stands(k - 1)))
        out["mixed"][key] = {"fleet_call_wall_ms": ms, "runs": runs,
                             "driving": int(sum(g.branch == N.BRANCH_ROLLOUT and g.ok == 1 for g in cycle.got)),
                             "at_goal": int(sum(g.branch == N.BRANCH_AT_GOAL for g in cycle.got))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="probes,plans,stop,drive,mixed")
    ap.add_argument("--lib", help="another build of the library")
    ap.add_argument("--ab", action="store_true", help="the probes leg of the shipped library and of libnavgpu_lpp.so (make tp-probe-ab)")
    args = ap.parse_args()
    if args.ab:
        lpp = os.path.join(os.path.dirname(N.lib_path()), "libnavgpu_lpp.so")
        if not os.path.exists(lpp):
            sys.exit(f"{lpp} is missing: make -C navigation_amd/csrc tp-probe-ab")
        base = [sys.executable, os.path.abspath(__file__), "--robots", str(args.robots), "--size", str(args.size), "--steps", str(args.steps),
                "--warmup", str(args.warmup), "--legs", "probes"]
        for name, extra in (("wave_per_probe", []), ("lane_per_probe", ["--lib", lpp])):
            r = subprocess.run(base + extra, capture_output=True, text=True, check=True)  # a fresh process per library
            print(json.dumps({name: json.loads(r.stdout.strip().splitlines()[-1])}))
        return
    if args.lib:
        N.lib_path = lambda: os.path.abspath(args.lib)
    import navigation_amd as nav
    fl, poses, plans = build(nav, args.robots, args.size)
    out = {"robots": args.robots, "size": args.size, "lib": os.path.basename(N.lib_path()),
           "timing": "median wall ms of the whole call(s), stream-synchronised", "steps": args.steps}
    legs = args.legs.split(",")
    if "probes" in legs:
        leg_probes(fl, poses, plans, args, out)
    if "plans" in legs:
        leg_plans(fl, poses, plans, args, out)
    if "stop" in legs:
        leg_cycle(fl, poses, plans, True, args, out)
    if "drive" in legs:
        leg_cycle(fl, poses, plans, False, args, out)
    if "mixed" in legs:
        leg_mixed(fl, poses, plans, args, out)
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
