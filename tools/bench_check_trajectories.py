#!/usr/bin/env python3
"""Time the batched checkTrajectory (navgpu_planner_check_trajectories, k_check_traj) and the control cycle that uses it, for 256 robots
at the benchmark's shape (bench.py's fleet: 400 x 400 maps, static + obstacle + inflation layers, 32 x 32 x 16 samples, 4-vertex footprint).

  --leg probes  the batched call with 1 and with 64 probes per robot against a loop of navgpu_planner_check_trajectory calls over the
                same probes, on the same build; the answers of the two are compared.  Device time is the library's profile bracket
                around k_check_traj (HIP events), wall time the whole call.
  --leg cycle   navgpu_local_planner_compute_velocity_commands with 0 %, 33 % and 100 % of the robots inside their goal tolerance
                (interleaved: every third robot), wall time per call.  A robot inside its tolerance carries a plan that ends where it
                stands, turned away from the goal heading and still moving: the stop branch, one checked candidate per cycle.  The
                others run the DWA cycle.

Nothing on this path had been measured before the batched call existed, so no figure is fixed anywhere: the comparison for the cycle leg
is against the PARENT commit.  Run  --leg cycle  from a checkout of the parent as well (the leg uses nothing the parent lacks; copy
this file into its tools/) and set the two JSON lines side by side.  Medians of --steps calls after --warmup."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from navigation_amd import _lib as N  # noqa: E402


def median_ms(call, steps, warmup):
    t = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return round(float(np.median(t)), 4)


def leg_probes(fl, n_robots, args, out):
    fl.update_map()
    fl.planner_cycle()
    fl.sync()
    fl.profile_select(["k_check_traj"])
    fl.profile(True)
    rs = np.random.RandomState(1)
    for per_robot in (1, 64):
        probes = np.stack([rs.uniform(0.0, 0.5, (n_robots, per_robot)), rs.uniform(-0.1, 0.1, (n_robots, per_robot)),
                           rs.uniform(-1.0, 1.0, (n_robots, per_robot))], 2).astype(np.float32)
        flat, off = probes.reshape(-1, 3), np.arange(n_robots + 1, dtype=np.uint32) * per_robot
        inst = np.arange(n_robots, dtype=np.uint32)
        dev = []

        def batched():
            fl.profile_reset()
            batched.ok = fl.check_trajectories(inst, flat, offsets=off)[0]
            dev.append(fl.profile_read()["k_check_traj"][0])

        def loop():
            loop.ok = np.array([fl.check_trajectory(i, probes[i, p]) for i in range(n_robots) for p in range(per_robot)])
        key = f"probes_{per_robot}_per_robot"
        out[key] = {"probes": n_robots * per_robot,
                    "batched_wall_ms": median_ms(batched, args.steps, args.warmup),
                    "batched_device_ms": round(float(np.median(dev[args.warmup:])), 4),
                    "single_call_loop_wall_ms": median_ms(loop, max(args.steps // 10, 3), 1)}
        out[key]["answers_differ"] = int((batched.ok != loop.ok).sum())
    fl.profile(False)


def leg_cycle(fl, insts, cfg, args, out):
    n_robots = len(insts)
    fl.update_map()
    fl.configure_local_planner(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, rot_stopped_vel=0.01, trans_stopped_vel=0.01,
                               max_rot_vel=cfg.max_rot_vel, min_rot_vel=cfg.min_rot_vel, acc_lim_x=cfg.acc_lim_x, acc_lim_y=cfg.acc_lim_y,
                               acc_lim_theta=cfg.acc_lim_theta, sim_period=cfg.sim_period, prune_plan=0, latch_xy_goal_tolerance=0)
    pose = np.array([[float(v) for v in ins["pos"]] for ins in insts])
    vel = np.array([[float(v) for v in ins["vel"]] for ins in insts])
    vel[:, 0] = np.maximum(vel[:, 0], 0.2)  # moving: a robot inside its tolerance takes the stop branch, every cycle
    s = np.linspace(1.0, 0.0, 21)
    for name, inside in (("0_percent", lambda k: False), ("33_percent", lambda k: k % 3 == 0), ("100_percent", lambda k: True)):
        for k, ins in enumerate(insts):
            if inside(k):  # a plan that ends where the robot stands, its goal heading 1 rad off the robot's
                th = pose[k, 2] + 1.0
                plan = np.stack([pose[k, 0] - s * np.cos(th), pose[k, 1] - s * np.sin(th), np.full_like(s, th)], 1)
            else:
                xy = np.asarray(ins["plan"], np.float64)
                plan = np.column_stack([xy, np.zeros(len(xy))])
            fl.set_global_plan(k, plan, None)
        branches = []

        def cycle():
            branches[:] = [r.branch for r in fl.compute_velocity_commands(pose, vel)]
        ms = median_ms(cycle, args.steps, args.warmup)
        out["cycle_" + name] = {"wall_ms": ms, "stop_or_rotate_robots": int(sum(b in (N.BRANCH_STOP, N.BRANCH_ROTATE) for b in branches)),
                                "dwa_robots": int(sum(b == N.BRANCH_DWA for b in branches))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", choices=["probes", "cycle", "both"], default="both")
    args = ap.parse_args()
    import bench
    import navigation_amd as nav
    fl, insts, cfg = bench.build_fleet(nav, args.robots, args.size, seed0=0)
    out = {"robots": args.robots, "size": args.size, "lib": os.path.basename(N.lib_path()),
           "timing": "median wall ms of the whole call; device = HIP events around k_check_traj",
           "compare": "the cycle leg is to be set against the same leg run from a checkout of the parent commit"}
    if args.leg in ("probes", "both"):
        leg_probes(fl, args.robots, args, out)
    if args.leg in ("cycle", "both"):
        leg_cycle(fl, insts, cfg, args, out)
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
