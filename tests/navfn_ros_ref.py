"""NavfnROS round its NavFn, restated in Python from the reference's lines (navfn/src/navfn_ros.cpp; costmap_2d/src/costmap_2d.cpp),
and the inputs the navfn_ros tests share.

  window_sequence        p = c - tol; while p <= c + tol: ...; p += resolution        navfn_ros.cpp:308-326, 140-151
  window_search          the tolerance search of makePlan                            :301-327
  window_search_loops    the same as the literal double loop (the tests compare the two)
  assemble               getPlanFromPotential's poses (+ best_pose)                  :440-456, 333-335
  make_plan              makePlan round a potential: oracle.pyoracle.navfn_plan by default    :218-374
  plan_from_potential    getPlanFromPotential                                        :400-461
  compute_potential      computePotential                                            :171-197
  point_potential / valid_point_potential                                            :130-169
  potential_cloud        the `potential` topic's points                              :342-368

Python floats are IEEE doubles: the sequences, sqrt and the costs are the reference's bits.  The second calcPath is
pyoracle.navfn_calc_path, whose limit is nx * ny / 2 where getPlanFromPotential's is nx * 4: calcPath's first k steps do not depend
on its limit and every step adds at most one point, so a path is found within nx * 4 steps exactly when it has <= nx * 4 points."""
import math

import numpy as np

from global_plan_ref import costmap_world_to_map, serpentine_cases

OK, START_OFF_MAP, GOAL_OFF_MAP, NO_PLAN, BORDER = range(5)
POT_HIGH = 1.0e10
DBL_MAX = float(np.finfo(np.float64).max)
MAX_WINDOW = 4096


def window_sequence(centre, tolerance, resolution):
    out = []
    p = centre - tolerance
    while p <= centre + tolerance:
        out.append(p)
        p += resolution
        assert len(out) <= MAX_WINDOW
    return out


def point_potential(pot, frame, x, y):
    """getPointPotential: a Python float (the float promoted), DBL_MAX off the map"""
    ny, nx = pot.shape
    c = costmap_world_to_map(x, y, float(frame[0]), float(frame[1]), float(frame[2]), nx, ny)
    return DBL_MAX if c is None else float(pot[c[1], c[0]])


def window_search(pot, frame, goal, tolerance, w_dist=1.0, w_len=0.0):
    """-> (candidates, best): best = dict(x, y, cost, cell, index) of the minimum of (cost, scan index), or None"""
    ny, nx = pot.shape
    ox, oy, res = (float(v) for v in frame)
    ys = window_sequence(goal[1], tolerance, res)
    xs = window_sequence(goal[0], tolerance, res)
    candidates, best = 0, None
    for iy, py in enumerate(ys):
        for ix, px in enumerate(xs):
            c = costmap_world_to_map(px, py, ox, oy, res, nx, ny)
            if c is None:
                continue
            potential = float(pot[c[1], c[0]])
            if not potential < POT_HIGH:
                continue
            candidates += 1
            dx, dy = px - goal[0], py - goal[1]
            cost = math.sqrt(dx * dx + dy * dy) * w_dist + potential * w_len
            if not cost < DBL_MAX:
                continue
            key = (cost, iy * len(xs) + ix)
            if best is None or key < (best["cost"], best["index"]):
                best = dict(x=px, y=py, cost=cost, cell=c, index=key[1])
    return candidates, best


def window_search_loops(pot, frame, goal, tolerance, w_dist=1.0, w_len=0.0):
    """navfn_ros.cpp:301-327 line by line -> (found_legal, best_cost, (x, y) of best_pose or None)"""
    resolution = float(frame[2])
    found_legal, best_cost, best_pose = False, DBL_MAX, None
    py = goal[1] - tolerance
    while py <= goal[1] + tolerance:
        px = goal[0] - tolerance
        while px <= goal[0] + tolerance:
            potential = point_potential(pot, frame, px, py)
            if potential < POT_HIGH:
                dx, dy = px - goal[0], py - goal[1]
                dist = math.sqrt(dx * dx + dy * dy)
                cost = dist * w_dist + potential * w_len
                if cost < best_cost:
                    found_legal, best_cost, best_pose = True, cost, (px, py)
            px += resolution
        py += resolution
    return found_legal, best_cost, best_pose


def assemble(path, frame, tail=None):
    """path: (n, 2) float32 as calcPath leaves it (start first) -> (n [+ 1], 3) float64 {x, y, yaw}"""
    ox, oy, res = (np.float64(v) for v in frame)
    p = np.asarray(path, np.float32).reshape(-1, 2)[::-1].astype(np.float64)
    poses = np.zeros((len(p), 3))
    poses[:, 0] = ox + p[:, 0] * res
    poses[:, 1] = oy + p[:, 1] * res
    if tail is not None:
        poses = np.concatenate([poses, np.asarray(tail, np.float64).reshape(1, 3)])
    return poses


def second_path(orc, pot, robot_cell, start_cell):
    """getPlanFromPotential's calcPath(nx * 4) -> (n, 2) float32, empty if none within the limit"""
    nx = pot.shape[1]
    path = orc.navfn_calc_path(pot, robot_cell, start_cell)
    return path if 0 < len(path) <= 4 * nx else np.zeros((0, 2), np.float32)


def make_plan(orc, cmap, frame, start, goal, tolerance, w_dist=1.0, w_len=0.0, allow_unknown=True, potential=None):
    """One plan.  potential: the array to search instead of the oracle's expansion (the wavefront test hands the device's over).
    -> dict(status, n_poses, poses, start_cell, goal_cell, found, cycles, potential, candidates, best, path, nav_start)"""
    ny, nx = cmap.shape
    ox, oy, res = (float(v) for v in frame)
    out = dict(status=OK, n_poses=0, poses=np.zeros((0, 3)), start_cell=None, goal_cell=None, found=False, cycles=0, potential=None,
               candidates=0, best=None, path=np.zeros((0, 2), np.float32), nav_start=None)
    sc = costmap_world_to_map(start[0], start[1], ox, oy, res, nx, ny)
    if sc is None:
        out["status"] = START_OFF_MAP
        return out
    out["start_cell"] = sc
    gc = costmap_world_to_map(goal[0], goal[1], ox, oy, res, nx, ny)
    if gc is None:
        if tolerance <= 0.0:
            out["status"] = GOAL_OFF_MAP
            return out
        gc = (0, 0)
    out["goal_cell"] = gc
    if potential is None:
        first, potential, cycles = orc.navfn_plan(cmap, sc, gc, cost_mode=1, allow_unknown=allow_unknown, astar=False, at_start=True)
        out.update(found=len(first) > 0, cycles=cycles)
    pot = np.asarray(potential, np.float32)
    candidates, best = window_search(pot, frame, goal, tolerance, w_dist, w_len)
    out.update(potential=pot, candidates=candidates, best=best, nav_start=gc, status=NO_PLAN)
    if best is None:
        return out
    out["nav_start"] = best["cell"]
    path = second_path(orc, pot, sc, best["cell"])
    if len(path) == 0:
        return out
    poses = assemble(path, frame, (best["x"], best["y"], goal[2]))
    out.update(status=OK, path=path, poses=poses, n_poses=len(poses))
    return out


def plan_from_potential(orc, pot, frame, goal, robot_cell):
    ny, nx = pot.shape
    gc = costmap_world_to_map(goal[0], goal[1], float(frame[0]), float(frame[1]), float(frame[2]), nx, ny)
    out = dict(status=GOAL_OFF_MAP, n_poses=0, poses=np.zeros((0, 3)), goal_cell=gc, path=np.zeros((0, 2), np.float32))
    if gc is None:
        return out
    path = second_path(orc, pot, robot_cell, gc)
    if len(path) == 0:
        out["status"] = NO_PLAN
        return out
    poses = assemble(path, frame)
    out.update(status=OK, path=path, poses=poses, n_poses=len(poses))
    return out


def compute_potential(orc, cmap, frame, point, allow_unknown=True):
    """-> (cell or None, potential or None, found)"""
    ny, nx = cmap.shape
    c = costmap_world_to_map(point[0], point[1], float(frame[0]), float(frame[1]), float(frame[2]), nx, ny)
    if c is None:
        return None, None, False
    path, pot, _ = orc.navfn_plan(cmap, c, (0, 0), cost_mode=1, allow_unknown=allow_unknown, astar=False, at_start=False)
    return c, pot, len(path) > 0


def valid_point_potential(pot, frame, point, tolerance):
    res = float(frame[2])
    for py in window_sequence(point[1], tolerance, res):
        for px in window_sequence(point[0], tolerance, res):
            if point_potential(pot, frame, px, py) < POT_HIGH:
                return True
    return False


def potential_cloud(pot, frame, start_cell):
    """-> (m, 4) float32 {x, y, z, pot_value}: float / float * 20 in float arithmetic, as written"""
    pot = np.asarray(pot, np.float32)
    ny, nx = pot.shape
    ox, oy, res = (np.float64(v) for v in frame)
    flat = pot.reshape(-1)
    keep = np.nonzero(flat.astype(np.float64) < 10e7)[0]
    out = np.zeros((len(keep), 4), np.float32)
    out[:, 0] = (ox + (keep % nx).astype(np.float64) * res).astype(np.float32)
    out[:, 1] = (oy + (keep // nx).astype(np.float64) * res).astype(np.float32)
    with np.errstate(all="ignore"):
        out[:, 2] = flat[keep] / pot[start_cell[1], start_cell[0]] * np.float32(20)
    out[:, 3] = flat[keep]
    return out


# ------------------------------------------------------------------------------------------------ the tests' inputs
RES = 0.05


def cell_pose(frame, cell, yaw, frac=(0.5, 0.5)):
    """a world pose inside the given cell"""
    return [frame[0] + (cell[0] + frac[0]) * frame[2], frame[1] + (cell[1] + frac[1]) * frame[2], yaw]


def _random_costmap(rs, n, density):
    """lethal cells at `density`, 15 % of the rest with a cost drawn from 1 .. 252, 1 % unknown (kept here so that the stored
    goldens' inputs depend on this file alone)"""
    cm = np.zeros((n, n), np.uint8)
    cm[rs.random_sample((n, n)) < density] = 254
    blur = (rs.random_sample((n, n)) < 0.15) & (cm == 0)
    cm[blur] = rs.randint(1, 253, blur.sum())
    cm[(rs.random_sample((n, n)) < 0.01) & (cm == 0)] = 255
    return cm


def _gp_case(rs, n):
    """a map with start and goal drawn 8 cells inside it in map coordinates, a 4 x 4 free patch round each"""
    cm = _random_costmap(rs, n, 0.03)
    start = rs.uniform(8, n - 9, 2)
    goal = rs.uniform(8, n - 9, 2)
    for x, y in (start, goal):
        cm[int(y) - 1:int(y) + 3, int(x) - 1:int(x) + 3] = 0
    return cm, start, goal


def random_cases(seeds=(31, 32, 33)):
    """48 x 48 maps (3 % lethal), two plans a seed, frames with origins from +-3 m at 0.05 m.
    -> list of (cmap, frame, start_xyyaw, goal_xyyaw)"""
    out = []
    for seed in seeds:
        rs = np.random.RandomState(seed)
        for _ in range(2):
            cm, s, g = _gp_case(rs, 48)
            frame = (float(rs.uniform(-3, 3)), float(rs.uniform(-3, 3)), RES)
            out.append((cm, frame, cell_pose(frame, (int(s[0]), int(s[1])), float(rs.uniform(-3, 3)), (s[0] % 1, s[1] % 1)),
                        cell_pose(frame, (int(g[0]), int(g[1])), float(rs.uniform(-3, 3)), (g[0] % 1, g[1] % 1))))
    return out


def blocked_goal_case():
    """the first random map with a 5 x 5 lethal blob round the goal's cell"""
    cm, frame, s, g = random_cases()[0]
    cm = cm.copy()
    gx, gy = int((g[0] - frame[0]) / frame[2]), int((g[1] - frame[1]) / frame[2])
    cm[gy - 2:gy + 3, gx - 2:gx + 3] = 254
    return cm, frame, s, g


def batch_cases():
    """The 48 x 48 handle of the parity test -> (list of (cmap, frame, start, goal, tolerance), list of expected statuses)"""
    rnd = random_cases()
    cm0, fr0, s0, g0 = rnd[0]
    ox, oy, res = fr0
    off_start = (cm0, fr0, [ox - 0.01, s0[1], 0.3], g0, 0.1)
    off_goal = [ox + 48 * res + 0.01, oy + 30.5 * res, 0.2]  # just off the map beside row 30
    blocked = blocked_goal_case()
    walled = cm0.copy()
    gc = (int((g0[0] - ox) / res), int((g0[1] - oy) / res))
    walled[gc[1] - 4, gc[0] - 4:gc[0] + 5] = walled[gc[1] + 4, gc[0] - 4:gc[0] + 5] = 254
    walled[gc[1] - 4:gc[1] + 5, gc[0] - 4] = walled[gc[1] - 4:gc[1] + 5, gc[0] + 4] = 254
    cases = [rnd[0] + (0.0,), off_start, rnd[1] + (0.1,), (cm0, fr0, s0, off_goal, 0.0), rnd[2] + (0.25,), (cm0, fr0, s0, off_goal, 0.3),
             blocked + (0.3,), rnd[3] + (0.0,), blocked + (0.0,), (walled, fr0, s0, g0, 0.1), rnd[4] + (-0.1,), rnd[5] + (0.15,)]
    statuses = [OK, START_OFF_MAP, OK, GOAL_OFF_MAP, OK, OK, OK, OK, NO_PLAN, NO_PLAN, NO_PLAN, OK]
    return cases, statuses


def ring_case():
    """48 x 48, free but for a 5 x 5 lethal blob whose centre cell holds the goal at its centre; tolerance 0.25.  Origin 0 and a
    resolution of 1/16 make the window's sums exact, so with weights (1, 0) the four candidates 3 cells from the goal along the
    axes tie exactly: the first in scan order, (0, -3), is the reference's."""
    cm = np.zeros((48, 48), np.uint8)
    cm[26:31, 28:33] = 254
    frame = (0.0, 0.0, 0.0625)
    return cm, frame, cell_pose(frame, (8, 9), 0.5), cell_pose(frame, (30, 28), -1.0), 0.25


def serpentine_case():
    """global_plan_ref.serpentine_cases' 64 x 64 map read as costmap_2d bytes, the robot in cell (2, 7), the goal in (62, 22), three
    corridors on: about as far as NavFn's max(nx * ny / 20, nx + ny) = 204 cycles reach on this map (the far corner of
    serpentine_cases is never reached), and more than 4 * 64 path points away.  -> (cmap, frame, start, goal)"""
    cm, frame, _, _ = serpentine_cases()[0]
    return cm, frame, cell_pose(frame, (2, 7), 0.4), cell_pose(frame, (62, 22), -2.9)


def pocket_case():
    """48 x 48: free but for a closed box of lethal cells whose inside (31 .. 41, 31 .. 41) nothing reaches"""
    cm = np.zeros((48, 48), np.uint8)
    cm[30, 30:43] = cm[42, 30:43] = 254
    cm[30:43, 30] = cm[30:43, 42] = 254
    frame = (-1.0, 0.5, RES)
    return cm, frame
