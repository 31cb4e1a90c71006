"""GlobalPlanner::makePlan around its core, restated in Python from the reference's lines (global_planner/src/planner_core.cpp,
orientation_filter.cpp; costmap_2d/src/costmap_2d.cpp), and the inputs the global-plan tests share.

  costmap_world_to_map   Costmap2D::worldToMap                         costmap_2d.cpp:208-220
  endpoints              makePlan up to clearRobotCell + the statuses  planner_core.cpp:250-286
  assemble               getPlanFromPotential + goal_copy              planner_core.cpp:351-395, 306-312
  orientation_filter     OrientationFilter::processPath on yaws        orientation_filter.cpp:53-111
  potential_grid         publishPotential's data                       planner_core.cpp:417-434
  make_plan              all of it round a core: oracle.pyoracle.global_planner_plan by default

Yaws stay yaws (the reference carries them through tf's quaternions; tools/global_plan_harness.cpp pins that round trip).
angles::shortest_angular_distance is the published fmod form of normalize_angle."""
import math

import numpy as np

NONE, FORWARD, INTERPOLATE, FORWARD_THEN_INTERPOLATE = range(4)
OK, START_OFF_MAP, GOAL_OFF_MAP, NO_PLAN, BORDER = range(5)
POT_HIGH = np.float32(1.0e10)


def costmap_world_to_map(wx, wy, origin_x, origin_y, resolution, nx, ny):
    if wx < origin_x or wy < origin_y:
        return None
    mx, my = int((wx - origin_x) / resolution), int((wy - origin_y) / resolution)
    return (mx, my) if mx < nx and my < ny else None


def endpoints(frame, start, goal, nx, ny, old_navfn_behavior=0):
    """-> (status, start_cell, goal_cell, start_xy, goal_xy): the cells and the double map coordinates makePlan plans with."""
    ox, oy, res = (float(v) for v in frame)
    sc = costmap_world_to_map(start[0], start[1], ox, oy, res, nx, ny)
    if sc is None:
        return START_OFF_MAP, None, None, None, None
    gc = costmap_world_to_map(goal[0], goal[1], ox, oy, res, nx, ny)
    if gc is None:
        return GOAL_OFF_MAP, sc, None, None, None
    if old_navfn_behavior:
        s, g = (float(sc[0]), float(sc[1])), (float(gc[0]), float(gc[1]))
    else:  # GlobalPlanner::worldToMap, convert_offset_ = 0.5; makePlan ignores what it returns
        s = ((start[0] - ox) / res - 0.5, (start[1] - oy) / res - 0.5)
        g = ((goal[0] - ox) / res - 0.5, (goal[1] - oy) / res - 0.5)
    inside = s[0] >= 2 and s[1] >= 2 and s[0] < nx - 3 and s[1] < ny - 3 and g[0] >= 1 and g[1] >= 1 and g[0] < nx - 1 and g[1] < ny - 1
    return (OK if inside else BORDER), sc, gc, s, g


def assemble(path, frame, goal, old_navfn_behavior=0):
    """path: (n, 2) float32, goal first, as the traceback leaves it -> (n_poses, 3) float64 {x, y, yaw} before the filter."""
    ox, oy, res = (np.float64(v) for v in frame)
    off = np.float64(0.0 if old_navfn_behavior else 0.5)
    p = np.asarray(path, np.float32)[::-1].astype(np.float64)
    poses = np.zeros((len(p), 3))
    poses[:, 0] = ox + (p[:, 0] + off) * res
    poses[:, 1] = oy + (p[:, 1] + off) * res
    g = np.asarray(goal, np.float64).reshape(1, 3)
    return np.concatenate([poses] + [g] * (2 if old_navfn_behavior else 1))


def normalize_angle(a):
    r = math.fmod(math.fmod(a, 2.0 * math.pi) + 2.0 * math.pi, 2.0 * math.pi)
    return r - 2.0 * math.pi if r > math.pi else r


def shortest_angular_distance(a, b):
    return normalize_angle(b - a)


def _interpolate(yaw, a, b):
    start_yaw, end_yaw = yaw[a], yaw[b]
    increment = shortest_angular_distance(start_yaw, end_yaw) / (b - a)
    for i in range(a, b + 1):
        yaw[i] = start_yaw + increment * i  # the absolute i, as written


def orientation_filter(poses, start_yaw, mode, info=None):
    """processPath on the yaw column of poses (in place).  info (a dict) receives the 0.35 search's index and smallest margin."""
    n = len(poses)
    yaw = [float(v) for v in poses[:, 2]]
    if mode in (FORWARD, FORWARD_THEN_INTERPOLATE):
        for i in range(n - 1):
            yaw[i] = math.atan2(poses[i + 1, 1] - poses[i, 1], poses[i + 1, 0] - poses[i, 0])
    if mode == INTERPOLATE:
        yaw[0] = float(start_yaw)
        _interpolate(yaw, 0, n - 1)
    if mode == FORWARD_THEN_INTERPOLATE:
        i, margin = 0, math.inf
        if n >= 3:  # (below that the reference reads before its array; the library takes 0)
            i = n - 3
            last = yaw[i]
            while i > 0:
                diff = abs(shortest_angular_distance(yaw[i - 1], last))
                margin = min(margin, abs(diff - 0.35))
                if diff > 0.35:
                    break
                i -= 1
        if info is not None:
            info.update(index=i, margin=margin)
        yaw[0] = float(start_yaw)
        _interpolate(yaw, i, n - 1)
    poses[:, 2] = yaw
    return poses


def potential_grid(pot, publish_scale):
    """-> ((ny, nx) int8, max as float32)"""
    pot = np.asarray(pot, np.float32)
    low = pot < POT_HIGH
    mx = np.float32(0.0)
    if low.any():
        mx = max(mx, pot[low].max())
    grid = np.full(pot.shape, -1, np.int8)
    if mx == 0:
        grid[~(pot >= POT_HIGH)] = 0  # (the reference divides by zero here)
    else:
        with np.errstate(over="ignore"):
            v = pot * np.float32(publish_scale) / mx  # float * int -> float, float / float
        keep = ~(pot >= POT_HIGH)
        grid[keep] = v[keep].astype(np.int32).astype(np.int8)
    return grid, mx


def make_plan(core, cmap, frame, start, goal, mode, info=None, **kw):
    """One plan.  core(cleared_cmap, start_xy, goal_xy, goal_cell, **kw) -> (path, potential): the expansion and traceback.
    -> dict(status, n_poses, poses, start_cell, goal_cell, path, potential)"""
    ny, nx = cmap.shape
    old = kw.get("old_navfn_behavior", 0)
    status, sc, gc, s, g = endpoints(frame, start, goal, nx, ny, old)
    out = dict(status=status, n_poses=0, poses=np.zeros((0, 3)), start_cell=sc, goal_cell=gc, path=None, potential=None)
    if status != OK:
        return out
    cm = np.array(cmap, np.uint8)
    cm[sc[1], sc[0]] = 0  # clearRobotCell
    path, pot = core(cm, s, g, gc, **kw)
    out.update(path=path, potential=pot)
    if len(path) == 0:
        out["status"] = NO_PLAN
        return out
    poses = orientation_filter(assemble(path, frame, goal, old), start[2], mode, info)
    out.update(n_poses=len(poses), poses=poses)
    return out


def oracle_core(orc):
    def core(cm, s, g, gc, **kw):
        path, pot, _, _ = orc.global_planner_plan(cm, s, g, gc, **kw)
        return path, pot
    return core


# ------------------------------------------------------------------------------------------------ the tests' inputs
def world_pose(frame, map_xy, yaw):
    """the world pose whose map coordinates (GlobalPlanner::worldToMap with convert_offset 0.5) are map_xy, up to rounding"""
    ox, oy, res = frame
    return [ox + (map_xy[0] + 0.5) * res, oy + (map_xy[1] + 0.5) * res, yaw]


def random_cases():
    """48 x 48 maps as tests/test_navfn.py draws them (_gp_case: 3 % lethal), seeds 21 - 23, two plans a seed; frames with the
    origin drawn from +-3 m at resolution 0.05.  -> list of (cmap, frame, start_xyyaw, goal_xyyaw)"""
    from test_navfn import _gp_case
    out = []
    for seed in (21, 22, 23):
        rs = np.random.RandomState(seed)
        for _ in range(2):
            cm, s, g = _gp_case(rs, 48)
            frame = (float(rs.uniform(-3, 3)), float(rs.uniform(-3, 3)), 0.05)
            out.append((cm, frame, world_pose(frame, s, float(rs.uniform(-3, 3))), world_pose(frame, g, float(rs.uniform(-3, 3)))))
    return out


def batch_cases():
    """The 48 x 48 handle of the parity test: the six random plans, and between them one plan each that is not attempted or finds
    nothing.  -> (list of cases, list of expected statuses)"""
    rnd = random_cases()
    cm0, fr0, s0, g0 = rnd[0]
    ox, oy, res = fr0
    off_start = (cm0, fr0, [ox - 0.01, s0[1], 0.3], g0)
    off_goal = (cm0, fr0, s0, [ox + 48 * res + 0.01, g0[1], 0.2])
    walled = cm0.copy()
    sc, gc = int((s0[0] - ox) / res), int((g0[0] - ox) / res)
    walled[:, (sc + gc) // 2] = 254
    border = (cm0, fr0, world_pose(fr0, (1.2, 20.0), 0.1), g0)
    cases = [rnd[0], off_start, rnd[1], rnd[2], off_goal, rnd[3], (walled, fr0, s0, g0), rnd[4], border, rnd[5]]
    statuses = [OK, START_OFF_MAP, OK, OK, GOAL_OFF_MAP, OK, NO_PLAN, OK, BORDER, OK]
    return cases, statuses


def serpentine_cases():
    """64 x 64: a wall every 6 rows with an 8-cell gap on alternating sides; the same map in two frames."""
    n = 64
    cm = np.zeros((n, n), np.uint8)
    for j, row in enumerate(range(9, n - 6, 6)):
        cm[row, :] = 254
        if j % 2 == 0:
            cm[row, n - 10:n - 2] = 0
        else:
            cm[row, 2:10] = 0
    out = []
    for frame, yaws in (((-1.25, 2.0, 0.05), (0.4, -2.9)), ((0.3125, -2.75, 0.1), (3.0, -3.0))):
        out.append((cm, frame, world_pose(frame, (4.3, 4.6), yaws[0]), world_pose(frame, (58.2, 59.4), yaws[1])))
    return out


def short_cases():
    """48 x 48, no obstacles: the goal 0 ... 2 cells from the start, for plans of a few poses."""
    cm = np.zeros((48, 48), np.uint8)
    frame = (1.5, -0.75, 0.05)
    out = []
    for k, d in enumerate((0.1, 0.45, 0.8, 1.2, 1.7, 2.1)):
        a = 0.7 + 1.1 * k
        s = (20.3, 24.4)
        g = (s[0] + d * math.cos(a), s[1] + d * math.sin(a))
        out.append((cm, frame, world_pose(frame, s, 1.0 - 0.5 * k), world_pose(frame, g, -2.0 + 0.9 * k)))
    return out
