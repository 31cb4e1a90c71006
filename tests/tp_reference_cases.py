"""The legacy TrajectoryPlanner reference fixture (tests/golden/g16_tp_reference.npz): its cases, the harness's input / output layouts
and a reader.

build_cases() is what tools/make_tp_goldens.py feeds tools/tp_reference_harness.cpp; load() / case() are what the tests read the
committed file with.  No oracle, no library and no reference tree in here: maps are hand-placed lethal cells, some inflated by
dwa_reference_cases.inflate (inputs only: any plausible costmap serves)."""
import json
import math
import os

import numpy as np

from dwa_reference_cases import INSCRIBED, LETHAL, NOINFO, RES, inflate  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_tp_reference.npz")
CFG_D = ("acc_lim_x", "acc_lim_y", "acc_lim_theta", "sim_time", "sim_granularity", "angular_sim_granularity", "pdist_scale", "gdist_scale",
         "occdist_scale", "heading_lookahead", "oscillation_reset_dist", "escape_reset_dist", "escape_reset_theta", "max_vel_x", "min_vel_x",
         "max_vel_th", "min_vel_th", "min_in_place_vel_th", "backup_vel", "sim_period", "heading_scoring_timestep")  # navgpu_tp_config order
CFG_I = ("vx_samples", "vtheta_samples", "holonomic_robot", "dwa", "heading_scoring", "simple_attractor", "meter_scoring")
N_CFG = len(CFG_D) + len(CFG_I) + 1 + 8
DEFAULTS = dict(acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2, sim_time=1.2, sim_granularity=0.05, angular_sim_granularity=0.05,
                pdist_scale=0.6, gdist_scale=0.8, occdist_scale=0.01, heading_lookahead=0.325, oscillation_reset_dist=0.05,
                escape_reset_dist=0.10, escape_reset_theta=math.pi / 2, max_vel_x=0.55, min_vel_x=0.0, max_vel_th=1.0, min_vel_th=-1.0,
                min_in_place_vel_th=0.4, backup_vel=-0.1, sim_period=0.05, heading_scoring_timestep=0.1, vx_samples=4, vtheta_samples=5,
                holonomic_robot=1, dwa=0, heading_scoring=0, simple_attractor=0, meter_scoring=0, y_vels=(-0.3, -0.1, 0.1, 0.3))
(STUCK_LEFT, STUCK_RIGHT, ROTATING_LEFT, ROTATING_RIGHT, STUCK_LEFT_STRAFE, STUCK_RIGHT_STRAFE, STRAFE_LEFT, STRAFE_RIGHT,
 ESCAPING) = (1 << k for k in range(9))  # navgpu_tp_state::flags
FORWARD, PAIR, IN_PLACE, Y_VELS, BACKUP = range(5)  # the five sampling stages of createTrajectories
N_CYC = N_CFG + 25
N_CALL = 8  # vx, vy, vtheta, cost_, points, the last point's x, y, theta (NaN without points)

FP4 = [[0.15, 0.15], [0.15, -0.15], [-0.15, -0.15], [-0.15, 0.15]]
FP5 = [[-0.14, -0.14], [-0.14, 0.14], [0.14, 0.14], [0.2, 0.0], [0.14, -0.14]]
FP2 = [[0.1, 0.0], [-0.1, 0.0]]
FP_WIDE = [[0.1, 0.3], [0.1, -0.3], [-0.1, -0.3], [-0.1, 0.3]]   # cannot turn in a 0.5 m corridor it stands across
FP_LONG = [[0.3, 0.1], [0.3, -0.1], [-0.3, -0.1], [-0.3, 0.1]]   # cannot turn in a 0.4 m pocket it stands along
PROBES = ((0.3, 0.0, 0.2), (0.0, 0.0, -0.8), (-0.1, 0.0, 0.0), (0.1, 0.1, 0.0))


def cfg_vector(cfg):
    y = list(cfg["y_vels"])
    assert len(y) <= 8
    return [float(cfg[k]) for k in CFG_D] + [int(cfg[k]) for k in CFG_I] + [len(y)] + y + [0.0] * (8 - len(y))


def cfg_dict(v):
    d = {k: float(x) for k, x in zip(CFG_D, v[:len(CFG_D)])}
    d.update({k: int(x) for k, x in zip(CFG_I, v[len(CFG_D):len(CFG_D) + len(CFG_I)])})
    n = int(v[len(CFG_D) + len(CFG_I)])
    d["y_vels"] = tuple(float(x) for x in v[N_CFG - 8:N_CFG - 8 + n])
    return d


def line(p0, p1, step=0.05):
    """Plan poses every `step` metres from p0 to p1 (both included)."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    n = max(1, int(round(float(np.hypot(*(p1 - p0))) / step)))
    return np.stack([p0 + (p1 - p0) * (k / n) for k in range(n + 1)])


def grid(nx, ny, origin, rects=()):
    """A costmap of free cells with lethal rectangles (world coordinates x0, y0, x1, y1; cells whose centre lies inside)."""
    cells = np.zeros((ny, nx), np.uint8)
    yy, xx = np.mgrid[0:ny, 0:nx]
    wx, wy = origin[0] + (xx + 0.5) * RES, origin[1] + (yy + 0.5) * RES
    for x0, y0, x1, y1 in rects:
        cells[(wx >= x0) & (wx <= x1) & (wy >= y0) & (wy <= y1)] = LETHAL
    return cells


def build_cases():
    """-> (cases, maps).  A case: name, map index, origin, allow_unknown, cfg, footprint, max_sim_steps (the fleet's), cycles.  A cycle:
    reconfigure (cfg or None), plan (None: keep), compute_dists, mode (0: pos / vel given, 1: advanced from the last command over dt),
    pos, vel, dt, pre (scoreTrajectory samples before findBestPath), post (scoreTrajectory / checkTrajectory samples after it)."""
    # No map here holds NO_INFORMATION cells.  TrajectoryPlanner, CostmapModel and MapGrid::setTargetCells take allow_unknown from
    # Costmap2D(costmap).getDefaultValue() (trajectory_planner.cpp:186, costmap_model.cpp:47, map_grid.cpp:106), and that copy never
    # sets default_value_ (costmap_2d.cpp:48, operator=): an uninitialised read.  What the reference does with unknown cells is therefore
    # not defined, and the harness refuses such maps.  The generator runs every case with both allow_unknown values and fails unless
    # the two records agree; the value a case names here is only the one the fixture's input array carries.
    maps, cases = [], []

    def cyc(pos=None, vel=(0, 0, 0), dt=0.2, plan=None, compute_dists=False, reconfigure=None, pre=(), post=()):
        return dict(reconfigure=reconfigure, plan=None if plan is None else np.asarray(plan, np.float64).reshape(-1, 2),
                    compute_dists=int(compute_dists), mode=int(pos is None), pos=np.asarray(pos if pos is not None else (0, 0, 0), np.float32),
                    vel=np.asarray(vel, np.float32), dt=float(dt), pre=np.asarray(pre, np.float64).reshape(-1, 3),
                    post=np.asarray(post, np.float64).reshape(-1, 3))

    def add(name, cells, origin, cfg, fp, cycles, allow_unknown=1, max_sim_steps=64):
        maps.append(np.ascontiguousarray(cells, np.uint8))
        c = dict(DEFAULTS)
        c.update(cfg)
        for k in cycles:
            if k["reconfigure"] is not None:
                r = dict(c)
                r.update(k["reconfigure"])
                k["reconfigure"] = r
        cases.append(dict(name=name, map=len(maps) - 1, origin=tuple(float(v) for v in origin), allow_unknown=int(allow_unknown), cfg=c,
                          fp=np.asarray(fp, np.float64), max_sim_steps=int(max_sim_steps), cycles=cycles))

    def follow(n, **kw):
        return [cyc(**kw) for _ in range(n)]

    # ---- open space, a non-square map with a negative origin: winners from the forward grid, the speed cap not binding
    org = (-1.0, -0.6)
    open_map = inflate(grid(96, 64, org, [(1.2, 0.9, 1.5, 1.3), (0.2, -0.3, 0.5, -0.1), (2.6, 0.2, 2.9, 0.5)]), inscribed=0.15)
    plan = line((0.313, 0.421), (3.2, 1.93))
    add("open_forward", open_map, org, dict(), FP4,
        [cyc((0.313, 0.421, 0.2), (0.2, 0.0, 0.1), plan=plan, compute_dists=True, pre=PROBES[:2], post=PROBES)] + follow(2, post=PROBES[:1]))
    # dwa, not holonomic, allow_unknown 0; a new, shorter plan in the third cycle: the final goal 0.3 m ahead caps max_vel_x
    add("dwa_short_plan", open_map, org, dict(dwa=1, holonomic_robot=0, vx_samples=5, vtheta_samples=6), FP5,
        [cyc((0.313, 0.421, 0.45), (0.3, 0.0, 0.0), plan=plan, post=PROBES[:2]), cyc(), cyc(plan=plan[:12], post=PROBES[:1]), cyc()],
        allow_unknown=0)
    # ---- the holonomic pair: the path runs beside the robot, only vtheta = 0 in the forward grid ((4, 1): dvtheta is x / 0)
    for name, side in (("pair_left", 1.0), ("pair_right", -1.0)):
        p = line((0.1, 0.4 + 0.3 * side), (3.0, 0.4 + 0.3 * side))
        add(name, open_map, org, dict(vx_samples=4, vtheta_samples=1, pdist_scale=2.0, max_vel_x=0.12), FP4,
            [cyc((0.613, 0.423, 0.0), (0.1, 0.0, 0.0), plan=p, post=PROBES[3:])] + follow(1))
    # ---- in-place rotation, each sign: the goal lies behind the robot
    big = inflate(grid(64, 64, (0.0, 0.0), [(0.4, 2.6, 0.8, 2.9)]), inscribed=0.15)
    for name, side in (("rotate_left", 1.0), ("rotate_right", -1.0)):
        p = line((1.613, 1.621), (0.45, 1.621 + 0.9 * side))
        add(name, big, (0.0, 0.0), dict(), FP4, [cyc((1.613, 1.621, 0.1 * side), plan=p)] + follow(5, dt=0.3, post=PROBES[1:2]))
    # the same start, with a reconfigure while stuck_left / rotating_left stand (the persistent state is kept), and meter_scoring on
    p = line((1.613, 1.621), (0.45, 2.521))
    add("rotate_reconfigure", big, (0.0, 0.0), dict(), FP4,
        [cyc((1.613, 1.621, 0.1), plan=p), cyc(dt=0.3), cyc(dt=0.3, reconfigure=dict(meter_scoring=1, occdist_scale=0.2, vtheta_samples=7)),
         cyc(dt=0.3, post=PROBES[:2])])
    # one theta sample: dvtheta is x / 0, so the gate of :669 turns down the in-place call, which costs what standing still costs
    add("gated_in_place", big, (0.0, 0.0), dict(vx_samples=4, vtheta_samples=1), FP4, [cyc((1.613, 1.621, 0.1), plan=p)] + follow(1))
    # nothing moves forward (max_vel_x = 0, not holonomic): every call costs what standing still costs and the in-place stage decides by
    # the goal distance ahead.  The theta window is -1 .. 0.8 in five samples (dvtheta = 0.45): -1, -0.55, -0.1, 0.35, 0.8.  The sample
    # 0.35 lies inside the gate of :669 and is clamped to min_in_place_vel_th = 0.6, above dvtheta; no other sample gives that call.  Its
    # last point faces 0.632 rad left of the start heading, which is where the goal lies, on the robot's row: the call has the smallest
    # goal distance ahead, and only the gate, read on the unclamped value, turns it down
    add("gate_decides", big, (0.0, 0.0), dict(holonomic_robot=0, max_vel_x=0.0, max_vel_th=0.8, min_in_place_vel_th=0.6), FP4,
        [cyc((1.613, 1.621, -0.632), plan=line((1.613, 1.621), (3.0, 1.621)))] + follow(1, dt=0.3))
    # the same standstill, seven samples, the goal off to the right on a diagonal: goal_map_ counts 4-connected steps, so several headings
    # have the same goal distance ahead, and the strict `<` of :679 keeps the first of them
    a = 0.1 - 0.45
    add("ahead_ties", big, (0.0, 0.0), dict(holonomic_robot=0, max_vel_x=0.0, vtheta_samples=7), FP4,
        [cyc((1.613, 1.621, 0.1), plan=line((1.613, 1.621), (1.613 + 1.4 * math.cos(a), 1.621 + 1.4 * math.sin(a))))])
    # ---- the y_vels stage, each sign, and the strafing flags: a wide robot across a corridor (no inflation: the corridor is 0.35 m),
    # min_vel_x > 0 so that nothing in the forward grid stands still.  The plan changes sides between cycles; the pose is held.
    cx, cy = 1.613, 1.621
    corridor = grid(64, 64, (0.0, 0.0), [(0.0, 0.4, cx - 0.233, 2.9), (cx + 0.137, 0.4, 3.2, 2.9)])
    up, down = line((cx, cy), (cx, 2.8)), line((cx, cy), (cx, 0.45))
    strafe = dict(min_vel_x=0.1, sim_time=1.7, heading_lookahead=0.0, oscillation_reset_dist=1.0)
    here = (cx, cy, 0.0)
    add("strafe_up_down_up", corridor, (0.0, 0.0), strafe, FP_WIDE,
        [cyc(here, plan=up, post=PROBES[3:]), cyc(here, plan=down), cyc(here, plan=up), cyc(here, plan=down)])
    add("strafe_down_up_down", corridor, (0.0, 0.0), strafe, FP_WIDE,
        [cyc(here, plan=down), cyc(here, plan=up), cyc(here, plan=down), cyc(here, plan=up)])
    # no path or goal term: the four y_vels calls cost the same (0), the `<=` of :768 lets each nearer one take over
    add("strafe_equal_costs", corridor, (0.0, 0.0), dict(strafe, pdist_scale=0.0, gdist_scale=0.0), FP_WIDE, [cyc(here, plan=up)])
    # the lookahead point 0.325 m ahead lies in the wall for every strafe: equal goal distances ahead (the obstacle cost), and the
    # strict `<` of :778 keeps the first legal call although the later ones are cheaper
    add("strafe_ahead_ties", corridor, (0.0, 0.0), dict(strafe, heading_lookahead=0.325), FP_WIDE, [cyc(here, plan=up)])
    # moving between the cycles, with a small oscillation_reset_dist: prev_x_ / prev_y_ follow the robot while it strafes, so the flag stands
    add("strafe_follow", corridor, (0.0, 0.0), dict(strafe, oscillation_reset_dist=0.05), FP_WIDE, [cyc(here, plan=up)] + follow(2, dt=0.5))
    # ---- backing up.  Boxed in by a lethal ring: -1 patched to 1.0, escape mode, cleared by distance
    ring = grid(64, 64, (0.0, 0.0))
    yy, xx = np.mgrid[0:64, 0:64]
    d = np.maximum(np.abs((xx + 0.5) * RES - 1.625), np.abs((yy + 0.5) * RES - 1.625))
    ring[(d > 0.17) & (d < 0.33)] = LETHAL
    add("boxed_in", ring, (0.0, 0.0), dict(), FP4,
        [cyc((1.613, 1.621, 0.3), plan=line((1.613, 1.621), (2.9, 2.4)), post=PROBES[:3])] + follow(4, dt=0.5))
    # an empty plan: every call -2, the backing up too: no escape mode, no command.  Then a plan that leaves the map.
    add("empty_plan", open_map, org, dict(), FP2,
        [cyc((0.313, 0.421, 0.2), plan=np.zeros((0, 2)), post=PROBES[:1]), cyc(), cyc(plan=line((0.313, 0.421), (4.4, 1.2)), post=PROBES[:1]), cyc()],
        allow_unknown=0)
    # a long robot in a dead-end pocket, not holonomic: backing up is legal; escape mode; out of the pocket it turns in place (the forward
    # stage is skipped) until escape_reset_theta clears the mode
    pocket = grid(64, 64, (0.0, 0.0), [(1.0, 1.80, 2.3, 1.95), (1.0, 1.30, 2.3, 1.45), (1.97, 1.30, 2.3, 1.95)])
    add("pocket_escape", pocket, (0.0, 0.0),
        dict(holonomic_robot=0, min_vel_x=0.1, sim_time=1.7, backup_vel=-0.3, escape_reset_dist=5.0, escape_reset_theta=0.4), FP_LONG,
        [cyc((1.613, 1.621, 0.0), plan=np.concatenate([line((1.613, 1.621), (0.6, 1.621)), line((0.6, 1.671), (0.6, 2.9))]))] +
        follow(9, dt=0.7, post=PROBES[2:3]))
    # ---- sample counts: (1, 5), then (1, 1) and (0, 0) through reconfigure (dvx, dvtheta are x / 0 or 0 / 0)
    add("sample_counts", open_map, org, dict(vx_samples=1, vtheta_samples=5), FP4,
        [cyc((0.313, 0.421, 0.2), (0.1, 0.0, 0.2), plan=plan), cyc((0.313, 0.421, 0.2), (0.1, 0.0, 0.2), reconfigure=dict(vx_samples=1, vtheta_samples=1)),
         cyc((0.313, 0.421, 0.2), (0.1, 0.0, 0.2), reconfigure=dict(vx_samples=0, vtheta_samples=0))])
    # ---- heading scoring.  The plan bends round a wall: its last poses are out of sight of the robot, the scan goes on to nearer ones
    wall = inflate(grid(80, 64, (0.0, 0.0), [(1.9, 0.0, 2.0, 2.2)]), radius=0.3, inscribed=0.1)
    bend = np.concatenate([line((0.813, 1.021), (0.813, 2.7)), line((0.863, 2.7), (3.2, 2.7)), line((3.2, 2.65), (3.2, 0.8))])
    hs = dict(heading_scoring=1, sim_time=1.25, sim_granularity=0.02, angular_sim_granularity=0.05)
    add("heading_bend", wall, (0.0, 0.0), hs, FP4,
        [cyc((0.813, 1.021, 0.9), (0.2, 0.0, 0.0), plan=bend, post=PROBES[:2]), cyc(),
         cyc(reconfigure=dict(heading_scoring_timestep=0.0), post=PROBES[:1]), cyc(reconfigure=dict(heading_scoring_timestep=5.0), post=PROBES[:1])],
        max_sim_steps=64)
    # nothing of the plan in sight: DBL_MAX
    add("heading_nothing_in_sight", wall, (0.0, 0.0), dict(hs, sim_granularity=0.05), FP4,
        [cyc((0.813, 1.021, 0.9), plan=line((3.2, 2.0), (3.2, 0.3)), post=PROBES[:1])])
    add("simple_attractor", open_map, org, dict(simple_attractor=1), FP5, [cyc((0.313, 0.421, 0.2), plan=plan, post=PROBES[:2])] + follow(1))
    # ---- the map's border: samples leave the map (-1), the heading_lookahead point of in-place calls lies off it; capacity just above
    # the longest call
    add("border", open_map, org, dict(), FP4, [cyc((3.8 - 0.213, 0.421, 0.0), (0.3, 0.0, 0.0), plan=plan, post=PROBES[:1])] + follow(1),
        max_sim_steps=22)
    # a two-point footprint: CostmapModel looks at the centre only, so the centre leaving the map is what generateTrajectory's own
    # worldToMap test (:272) sees first
    add("fp2_off_border", open_map, org, dict(), FP2, [cyc((3.8 - 0.113, 0.421, 0.0), (0.3, 0.0, 0.0), plan=plan, post=PROBES[:1])])
    # a footprint vertex off the map at the start pose: getFootprintCells returns before the fill
    add("vertex_off_map", open_map, org, dict(), FP4, [cyc((-1.0 + 0.113, 0.421, 0.0), plan=plan)])
    # lethal cells under the robot: within_robot lets the wavefront through them
    # (not under its centre: goal_map_ has no within_robot marks, a robot whose own cell is lethal scores -2 everywhere)
    under = open_map.copy()
    under[21, 27] = LETHAL  # world (0.35 .. 0.4, 0.45 .. 0.5): inside the outline at every heading
    under[20, 26] = 200     # the robot's own cell, dearer than anything under the outline: the centre cell's cost is the occ_cost (:307)
    add("lethal_under_robot", under, org, dict(), FP5, [cyc((0.313, 0.421, 0.0), plan=plan, compute_dists=True, pre=PROBES[:1], post=PROBES[1:2])])
    return cases, maps


def encode_input(c, shape):
    d = [shape[1], shape[0], RES, c["origin"][0], c["origin"][1], 255 if c["allow_unknown"] else 0, len(c["fp"]), len(c["cycles"])]
    d += cfg_vector(c["cfg"]) + list(np.asarray(c["fp"], np.float64).ravel())
    for k in c["cycles"]:
        d += [int(k["reconfigure"] is not None)] + (cfg_vector(k["reconfigure"]) if k["reconfigure"] is not None else [])
        d += [-1 if k["plan"] is None else len(k["plan"]), k["compute_dists"]] + ([] if k["plan"] is None else list(k["plan"].ravel()))
        d += [k["mode"]] + [float(v) for v in k["pos"]] + [float(v) for v in k["vel"]] + [k["dt"]]
        d += [len(k["pre"])] + list(k["pre"].ravel()) + [len(k["post"])] + list(k["post"].ravel())
    return np.asarray(d, np.float64)


def decode_input(d):
    """The inverse of encode_input: a case dict (without name / map / max_sim_steps) from the fixture's NAME_in."""
    n_fp, n_cycles = int(d[6]), int(d[7])
    c = dict(size_x=int(d[0]), size_y=int(d[1]), res=float(d[2]), origin=(float(d[3]), float(d[4])), allow_unknown=int(d[5] != 0),
             cfg=cfg_dict(d[8:8 + N_CFG]), fp=d[8 + N_CFG:8 + N_CFG + 2 * n_fp].reshape(-1, 2).copy(), cycles=[])
    at = 8 + N_CFG + 2 * n_fp
    for _ in range(n_cycles):
        k = dict(reconfigure=None)
        if d[at]:
            k["reconfigure"] = cfg_dict(d[at + 1:at + 1 + N_CFG])
            at += N_CFG
        at += 1
        n_plan, k["compute_dists"] = int(d[at]), int(d[at + 1])
        at += 2
        k["plan"] = None
        if n_plan >= 0:
            k["plan"] = d[at:at + 2 * n_plan].reshape(-1, 2).copy()
            at += 2 * n_plan
        k["mode"], k["dt"] = int(d[at]), float(d[at + 7])
        k["pos"], k["vel"] = d[at + 1:at + 4].astype(np.float32), d[at + 4:at + 7].astype(np.float32)
        at += 8
        for key in ("pre", "post"):
            n = int(d[at])
            k[key] = d[at + 1:at + 1 + 3 * n].reshape(-1, 3).copy()
            at += 1 + 3 * n
        c["cycles"].append(k)
    assert at == len(d)
    return c


def decode_output(o, c, shape):
    """The harness's doubles of one case -> the fixture's arrays and the measured boundary margin."""
    rows, calls, traj, within, grids, pre, post = [], [], [], [], [], [], []
    cells = shape[0] * shape[1]
    at = 0
    for _ in c["cycles"]:
        head = list(o[at:at + N_CFG + 6])
        at += N_CFG + 6
        n_pre = int(o[at])
        pre.append(o[at + 1:at + 1 + n_pre])
        at += 1 + n_pre
        n_calls = int(o[at])
        calls.append(o[at + 1:at + 1 + N_CALL * n_calls].reshape(-1, N_CALL))
        at += 1 + N_CALL * n_calls
        winner = list(o[at:at + 6])
        n_points = int(winner[4])
        at += 6
        traj.append(o[at:at + 3 * n_points].reshape(-1, 3))
        at += 3 * n_points
        tail = list(o[at:at + 9])  # drive[3], flags, five state doubles
        at += 9
        n_within = int(o[at])
        within.append(o[at + 1:at + 1 + n_within].astype(np.int32))
        at += 1 + n_within
        g = o[at:at + 2 * cells]
        at += 2 * cells
        assert g.max() <= 65535 and np.array_equal(g, np.floor(g))
        grids.append(g.astype(np.uint16).reshape(2, shape[0], shape[1]))
        n_post = int(o[at])
        post.append(o[at + 1:at + 1 + 2 * n_post].reshape(-1, 2))
        at += 1 + 2 * n_post
        rows.append(head + [n_pre, n_calls] + winner + tail + [n_within, n_post])
    margin = float(o[at])
    assert at + 2 == len(o)  # the last double, allow_unknown_ as the planner read it, is an uninitialised read: not kept
    out = dict(cyc=np.asarray(rows, np.float64), call=np.concatenate(calls), traj=np.concatenate(traj), within=np.concatenate(within),
               grid=np.stack(grids), pre=np.concatenate(pre), post=np.concatenate(post))
    assert out["cyc"].shape[1] == N_CYC
    return out, margin


class Cycle:
    """One cycle of a case, unpacked: the inputs, the configuration the reference held, and what it computed."""

    def __init__(self, inp, row, calls, traj, within, grid, pre, post, entry_flags):
        self.reconfigure, self.plan, self.compute_dists = inp["reconfigure"] is not None, inp["plan"], inp["compute_dists"]
        self.pre_samples, self.post_samples = inp["pre"], inp["post"]
        self.cfg = cfg_dict(row[:N_CFG])
        r = row[N_CFG:]
        self.pos, self.vel = r[0:3].astype(np.float32), r[3:6].astype(np.float32)
        self.calls = calls                       # a row of N_CALL per generateTrajectory call
        self.winner_vel, self.cost, self.n_points, self.best_call = r[8:11], float(r[11]), int(r[12]), int(r[13])
        self.drive, self.flags, self.state = r[14:17], int(r[17]), r[18:23]
        self.traj, self.within, self.grid, self.pre, self.post = traj, within, grid, pre, post
        self.entry_flags = entry_flags           # the flags this cycle found (those the cycle before left)

    def stage_of(self, index):
        """Which sampling stage of createTrajectories made call `index`: by position, from the counts the reference held."""
        c = self.cfg
        bounds = [] if self.entry_flags & ESCAPING else [(FORWARD, c["vx_samples"] * c["vtheta_samples"]), (PAIR, 2 * c["holonomic_robot"])]
        bounds.append((IN_PLACE, c["vtheta_samples"]))
        at = 0
        for stage, n in bounds:
            at += n
            if index < at:
                return stage
        # the y_vels stage, where it is reached, makes all its calls; one more call is the backing up
        return Y_VELS if c["holonomic_robot"] and index < at + len(c["y_vels"]) else BACKUP

    def stage_calls(self, stage):
        return [i for i in range(len(self.calls)) if self.stage_of(i) == stage]


def unpack(c, rec):
    out, at = [], dict(call=0, traj=0, within=0, pre=0, post=0)
    flags = 0
    for k, inp in enumerate(c["cycles"]):
        row = rec["cyc"][k]
        r = row[N_CFG:]
        n = dict(pre=int(r[6]), call=int(r[7]), traj=int(r[12]), within=int(r[23]), post=int(r[24]))
        part = {key: rec[key][at[key]:at[key] + n[key]] for key in n}
        out.append(Cycle(inp, row, part["call"], part["traj"], part["within"], rec["grid"][k], part["pre"], part["post"], flags))
        flags = out[-1].flags
        for key in n:
            at[key] += n[key]
    assert all(at[key] == len(rec[key]) for key in at)
    return out


def load():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["meta"]))


def case(g, meta, name):
    """-> (case dict, costmap, list of Cycle)"""
    c = decode_input(g[name + "_in"])
    c["name"] = name
    c["max_sim_steps"] = meta["fleet"][name]["max_sim_steps"]
    rec = {k: g[f"{name}_{k}"] for k in ("cyc", "call", "traj", "within", "grid", "pre", "post")}
    return c, g[f"map_{int(g[name + '_map'])}"], unpack(c, rec)
