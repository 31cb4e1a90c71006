#!/usr/bin/env python3
"""Time per-robot limits (navgpu_planner_set_limits) for 256 robots at the benchmark's shape (bench.py's fleet: 400 x 400 maps, static +
obstacle + inflation layers, 32 x 32 x 16 samples, 4-vertex footprint).

  --leg call    what it costs to slow robots down while the fleet drives: set_limits for 1 robot and for every third robot (85 calls
                of one record each), against navgpu_planner_configure of the whole fleet - the only way to change a limit on a build
                without the call, and one that changes every robot.  Each call is timed BEHIND a queued planner cycle, as a recovery
                behaviour or a reconfigure callback meets the fleet: a call that waits for the stream pays for that cycle.
  --leg cycle   the planner cycle (stage_poses + planner_cycle + results, wall time) of a fleet with three interleaved limit classes -
                the configuration's own, MoveSlowAndClear's 0.25 m/s / 0.45 rad/s, and one faster in every field - against the same
                fleet with uniform limits, before and after.

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

CONTROL = dict(xy_goal_tolerance=0.1, yaw_goal_tolerance=0.05, trans_stopped_vel=0.1, rot_stopped_vel=0.1, prune_plan=1)


def median_ms(call, steps, warmup, before=None):
    t = []
    for i in range(warmup + steps):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if i >= warmup:
            t.append((t1 - t0) * 1e3)
    return round(float(np.median(t)), 4)


def limits_of(cfg, **kw):
    return dict({n: getattr(cfg, n) for n in N.RobotLimits.FIELDS[:11]}, **dict(CONTROL, **kw))


def leg_call(fl, cfg, n, args, out):
    fl.update_map()
    slow, own = limits_of(cfg, max_trans_vel=0.25, max_rot_vel=0.45), limits_of(cfg)
    flip = [0]

    def queue_cycle():  # a cycle is queued and still runs when the timed call begins
        fl.sync()
        fl.planner_cycle()

    def one_robot():
        flip[0] ^= 1
        fl.set_limits([slow if flip[0] else own], first=n // 2)

    def every_third():
        flip[0] ^= 1
        rec = N.RobotLimits(**{k: (int(v) if k == "prune_plan" else float(v)) for k, v in (slow if flip[0] else own).items()})
        arr = (N.RobotLimits * 1)(rec)
        for i in range(0, n, 3):
            fl.set_limits(arr, first=i)

    def configure():
        fl.configure_planner(cfg)

    out["call"] = {"set_limits_1_robot_wall_ms": median_ms(one_robot, args.steps, args.warmup, queue_cycle),
                   "set_limits_every_third_robot_wall_ms": median_ms(every_third, args.steps, args.warmup, queue_cycle),
                   "planner_configure_wall_ms": median_ms(configure, args.steps, args.warmup, queue_cycle),
                   "queued_cycle_alone_wall_ms": median_ms(fl.sync, args.steps, args.warmup, queue_cycle)}
    fl.sync()


def leg_cycle(fl, insts, cfg, n, args, out):
    fl.update_map()
    pos, vel = np.stack([i["pos"] for i in insts]), np.stack([i["vel"] for i in insts])
    res = (N.PlanResult * n)()

    def cycle():
        fl.stage_poses(pos, vel)
        fl.planner_cycle()
        fl.results_into(res)

    classes = [limits_of(cfg), limits_of(cfg, max_trans_vel=0.25, max_rot_vel=0.45),
               limits_of(cfg, max_trans_vel=cfg.max_trans_vel * 1.5, max_vel_x=cfg.max_vel_x * 1.5, min_vel_x=-0.2, max_vel_y=0.2, min_vel_y=-0.2,
                         max_rot_vel=cfg.max_rot_vel * 1.5, acc_lim_x=cfg.acc_lim_x * 1.4, acc_lim_y=cfg.acc_lim_y * 1.4,
                         acc_lim_theta=cfg.acc_lim_theta * 1.4)]
    r = {"uniform_wall_ms": median_ms(cycle, args.steps, args.warmup)}
    fl.set_limits([classes[i % 3] for i in range(n)])
    r["three_classes_wall_ms"] = median_ms(cycle, args.steps, args.warmup)
    r["three_classes_valid_robots"] = int(sum(x.cost >= 0 for x in res))
    fl.configure_planner(cfg)  # every record the configuration's again (the window stays planned for the fastest class)
    r["uniform_again_wall_ms"] = median_ms(cycle, args.steps, args.warmup)
    r["uniform_valid_robots"] = int(sum(x.cost >= 0 for x in res))
    out["cycle"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", choices=["call", "cycle", "both"], default="both")
    args = ap.parse_args()
    import bench
    import navigation_amd as nav
    fl, insts, cfg = bench.build_fleet(nav, args.robots, args.size, seed0=0)
    out = {"robots": args.robots, "size": args.size, "lib": os.path.basename(N.lib_path()), "timing": "median wall ms of the whole call"}
    if args.leg in ("call", "both"):
        leg_call(fl, cfg, args.robots, args, out)
    if args.leg in ("cycle", "both"):
        leg_cycle(fl, insts, cfg, args.robots, args, out)
    fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
