"""What the trajectory-cloud tests share: the scenes, and restatements of the reference code navgpu_planner_trajectory_cloud and
navgpu_planner_sample_terms replace - used by tests/test_traj_cloud_model.py (which pins the model on the CPU oracle) and
tests/test_gpu_traj_cloud.py (which compares the device against them):

  expected_cloud   the loop of DWAPlanner::findBestPath over all_explored (dwa_local_planner/src/dwa_planner.cpp:318-348): every
                   point of every scored slot whose cost is >= 0, as MapGridCostPoint's seven floats
  incumbents       the best cost SimpleScoredSamplingPlanner::findBestTrajectory holds when it scores slot i
                   (simple_scored_sampling_planner.cpp:111-127), as the exclusive prefix minimum of the full costs
  replay_cost_ref  SimpleScoredSamplingPlanner::scoreTrajectory (:50-79) from a slot's raw critic values
Nothing here reads the product."""
import math

import numpy as np

N_CELLS = 160
RES = 0.05
FOOTPRINT = np.array([[0.2, 0.2], [0.2, -0.2], [-0.2, -0.2], [-0.2, 0.2]], np.float64)
MAX_SIM_STEPS = 64
SAMPLES = dict(vx_samples=16, vy_samples=8, vth_samples=10, min_vel_x=-0.2)  # 1584 - 1683 slots; backwards samples for the oscillation critic
BY_TIME = dict(discretize_by_time=1, sim_time=2.0, sim_granularity=0.1)  # 20 points per slot
BY_DISTANCE = dict(discretize_by_time=0)                                  # 6 ... ~40 points, the all-zero sample rejected
OSC_FORWARD_POS_ONLY = 1 << 8


def config_kw(by_time=True, **kw):
    d = dict(SAMPLES)
    d.update(BY_TIME if by_time else BY_DISTANCE)
    d.update(kw)
    return d


def _plan(x0, y0, heading, n=120, step=0.03):
    i = np.arange(n, dtype=np.float64)
    return np.stack([x0 + step * i * math.cos(heading), y0 + step * i * math.sin(heading) + 0.2 * np.sin(0.05 * i)], axis=1)


def scene(name):
    """-> dict(master uint8 [160, 160], pos, vel float32 [3], plan float64 [n, 2])"""
    n = N_CELLS
    c = n * RES / 2.0
    m = np.zeros((n, n), np.uint8)
    cx = cy = n // 2
    if name == "band":  # the robot faces away from its plan, a band of INSCRIBED cells ahead of it: legal for the footprint, an obstacle for the path grid
        m[:, cx - 25:cx - 7] = 253
        return dict(master=m, pos=np.array([c, c, math.pi], np.float32), vel=np.array([0.15, 0.0, 0.0], np.float32), plan=_plan(c, c, 0.0))
    if name == "posts":  # lethal posts around the robot, 9 cells away (tests/test_gpu_parity_r4.py): most slots fail the obstacle critic
        for dy in range(-30, 31, 6):
            for dx in range(-30, 31, 6):
                if max(abs(dx), abs(dy)) >= 9:
                    m[cy + dy, cx + dx] = 254
        return dict(master=m, pos=np.array([c, c, 0.4], np.float32), vel=np.array([0.25, 0.0, 0.1], np.float32), plan=_plan(c, c, 0.3))
    if name == "open":  # low-cost clutter and a lethal wall to one side
        m[cy - 40:cy + 40, cx - 40:cx + 40] = 37
        m[cy + 14, cx - 30:cx + 30] = 254
        return dict(master=m, pos=np.array([c, c, 0.9], np.float32), vel=np.array([0.05, 0.0, -0.1], np.float32), plan=_plan(c, c, 0.5))
    if name == "near_goal":  # within forward_point_distance of the end of the plan: the alignment critic is switched off
        m[cy - 40:cy + 40, cx - 40:cx + 40] = 11
        p = _plan(c - 0.9, c, 0.0, n=36, step=0.03)
        return dict(master=m, pos=np.array([p[-1, 0] - 0.12, p[-1, 1] + 0.05, 0.2], np.float32), vel=np.array([0.1, 0.0, 0.0], np.float32), plan=p)
    raise KeyError(name)


def oracle_planner(orc, sc, cfg_kw):
    p = orc.DwaPlanner(sc["master"], RES, 0.0, 0.0, orc.DwaConfig(**cfg_kw))
    p.set_plan()
    return p


def oracle_cycle(orc, p, sc, pos=None, vel=None):
    """one findBestPath on the oracle -> dict(result, cref, cfull, status, samples, pos, vel)"""
    pos = sc["pos"] if pos is None else np.asarray(pos, np.float32)
    vel = sc["vel"] if vel is None else np.asarray(vel, np.float32)
    res, _, cref, cfull, status = p.cycle(pos, vel, sc["plan"], FOOTPRINT)
    return dict(result=res, cref=cref, cfull=cfull, status=status, samples=p.samples(), pos=pos, vel=vel, cfg=p.cfg)


def orc_points(orc, cyc, i):
    """points of slot i's trajectory"""
    return orc.generate_trajectory(cyc["cfg"], cyc["pos"], cyc["vel"], cyc["samples"][i])[0]


def incumbents(cfull, status):
    """best_i = min { full_j : j < i, slot j scored, full_j >= 0 }, -1 when there is no such slot"""
    best = np.full(len(cfull), -1.0)
    cur = -1.0
    for i in range(len(cfull)):
        best[i] = cur
        if status[i] == 1 and cfull[i] >= 0 and (cur < 0 or cfull[i] < cur):
            cur = cfull[i]
    return best


def replay_cost_ref(critic, first_fail, scales, best):
    """scoreTrajectory (:50-79) for one scored slot: critic = the five raw values in critic order behind the oscillation critic (the
    failing one holds its code), scales likewise; fp64 sums in the reference's order"""
    if first_fail == 0:
        return -5.0
    total = np.float64(0.0)
    for k in range(5):
        if scales[k] == 0:
            continue
        cost = np.float64(critic[k])
        if cost < 0:
            return float(cost)
        if cost != 0:
            cost = cost * np.float64(scales[k])
        total = total + cost
        if best > 0 and total > best:
            break
    return float(total)


def expected_cloud(orc, cyc, costs):
    """the cloud of one cycle for per-slot costs `costs` (cref: the reference's; cfull: the order-independent one) ->
    (points [n, 7] float32, member [slots] bool, n_points [slots], offset [slots])"""
    status, samples = cyc["status"], cyc["samples"]
    pts, member, n_points, offset = [], np.zeros(len(status), bool), np.zeros(len(status), np.int64), np.zeros(len(status), np.int64)
    at = 0
    for i in range(len(status)):
        offset[i] = at
        if status[i] != 1:
            continue
        k, xyth, _ = orc.generate_trajectory(cyc["cfg"], cyc["pos"], cyc["vel"], samples[i])
        n_points[i] = max(k, 0)
        if costs[i] < 0:
            continue
        member[i] = True
        p = np.zeros((k, 7), np.float32)
        p[:, 0] = xyth[:, 0]  # pt.x = p_x: double -> float (dwa_planner.cpp:339-343)
        p[:, 1] = xyth[:, 1]
        p[:, 3] = xyth[:, 2]  # pt.path_cost = p_th
        p[:, 6] = np.float32(costs[i])
        pts.append(p)
        at += k
    return (np.concatenate(pts) if pts else np.zeros((0, 7), np.float32)), member, n_points, offset
