#!/usr/bin/env python3
"""Time the control cycle (navgpu_local_planner_compute_velocity_commands) when the robots inside their goal tolerance are scattered among
the driving ones, for 256 robots at the benchmark's shape (bench.py's fleet: 400 x 400 maps, static + obstacle + inflation layers,
32 x 32 x 16 samples, 4-vertex footprint).

  --leg cycle   the control cycle with 0 %, 33 % (every third robot), 50 % (alternating) and 100 % of the robots inside their tolerance,
                wall time per call.  A robot inside its tolerance carries a plan that ends where it stands, turned away from the goal
                heading and still moving: the stop branch, one checked candidate per cycle.  The others run the DWA cycle - as one
                contiguous range at 0 %, as 85 / 128 runs at 33 % / 50 %, which a build with navgpu_planner_cycle_list hands over as one
                list.
  --leg kernels the whole-fleet planner cycle through the range calls and through the listed calls with the list {0 .. n-1}, on the same
                build: what the indirection costs a cycle that does not need it.  Skipped on a build without the listed calls.

The control cycle is a public call every build has: the comparison for the cycle leg is against the PARENT commit.  Run  --leg cycle  from a
checkout of the parent as well (copy this file into its tools/) and set the JSON lines side by side, two runs of each, interleaved.
Medians of --steps calls after --warmup."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from navigation_amd import _lib as N  # noqa: E402

SHARES = (("0_percent", lambda k: False), ("33_percent", lambda k: k % 3 == 0), ("50_percent", lambda k: k % 2 == 0),
          ("100_percent", lambda k: True))


def median_ms(call, steps, warmup):
    t = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return round(float(np.median(t)), 4)


def leg_cycle(fl, insts, cfg, args, out):
    fl.update_map()
    fl.configure_local_planner(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, rot_stopped_vel=0.01, trans_stopped_vel=0.01,
                               max_rot_vel=cfg.max_rot_vel, min_rot_vel=cfg.min_rot_vel, acc_lim_x=cfg.acc_lim_x, acc_lim_y=cfg.acc_lim_y,
                               acc_lim_theta=cfg.acc_lim_theta, sim_period=cfg.sim_period, prune_plan=0, latch_xy_goal_tolerance=0)
    pose = np.array([[float(v) for v in ins["pos"]] for ins in insts])
    vel = np.array([[float(v) for v in ins["vel"]] for ins in insts])
    vel[:, 0] = np.maximum(vel[:, 0], 0.2)  # moving: a robot inside its tolerance takes the stop branch, every cycle
    s = np.linspace(1.0, 0.0, 21)
    for name, inside in SHARES:
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
        dwa = [b == N.BRANCH_DWA for b in branches]
        out["cycle_" + name] = {"wall_ms": ms, "stop_or_rotate_robots": int(sum(b in (N.BRANCH_STOP, N.BRANCH_ROTATE) for b in branches)),
                                "dwa_robots": int(sum(dwa)), "dwa_runs": int(sum(d and (k == 0 or not dwa[k - 1]) for k, d in enumerate(dwa)))}


def leg_kernels(fl, n_robots, args, out):
    if not hasattr(fl, "planner_cycle_list"):
        out["kernels"] = "this build has no listed cycle"
        return
    fl.update_map()
    everyone = np.arange(n_robots, dtype=np.uint32)
    res = (N.PlanResult * n_robots)()

    def by_range():
        fl.planner_cycle()
        fl.results_into(res)

    def by_list():
        fl.planner_cycle_list(everyone)
        fl.results_into(res)
    out["kernels"] = {"range_cycle_wall_ms": median_ms(by_range, args.steps, args.warmup),
                      "listed_cycle_wall_ms": median_ms(by_list, args.steps, args.warmup),
                      "range_cycle_again_wall_ms": median_ms(by_range, args.steps, args.warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", choices=["cycle", "kernels", "both"], default="both")
    args = ap.parse_args()
    import bench
    import navigation_amd as nav
    fl, insts, cfg = bench.build_fleet(nav, args.robots, args.size, seed0=0)
    out = {"robots": args.robots, "size": args.size, "lib": os.path.basename(N.lib_path()),
           "timing": "median wall ms of the whole call",
           "compare": "the cycle leg is to be set against the same leg run from a checkout of the parent commit"}
    if args.leg in ("kernels", "both"):
        leg_kernels(fl, args.robots, args, out)
    if args.leg in ("cycle", "both"):
        leg_cycle(fl, insts, cfg, args, out)
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
