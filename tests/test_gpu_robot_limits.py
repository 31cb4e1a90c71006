"""Per-robot velocity and acceleration limits (navgpu_planner_set_limits / _get_limits): a fleet whose robots own their
LocalPlannerLimits, as every robot of the reference does.  Need a real MI355X.

Yardsticks:
  (a) twin fleets - a uniform fleet configured FLEET-WIDE with limit class L_j on the same maps, poses, plans and footprints: a robot
      with L_j in the mixed fleet equals robot for robot its twin bit for bit (the same arithmetic on the same inputs: no tolerance);
  (b) the DWA oracle, one planner object per robot built with that robot's own configuration: winner and failure codes exact, costs
      within 1e-5, the bounds of tests/test_gpu_parity.py.
Maps are 64 x 64 at 0.05 m with seeded obstacles near the robot and a wall; samples 6 x 3 x 8 with a holonomic y axis."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwa_reference_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

NAVGPU_ERR_INVALID, NAVGPU_ERR_HIP, NAVGPU_ERR_CAPACITY = -1, -3, -4
SIZE, MAX_PLAN = 64, 64
CFG = dict(D.DEFAULTS, vx_samples=6, vy_samples=3, vth_samples=8, sim_time=1.0, sim_granularity=0.1, use_dwa=1, discretize_by_time=1,
           rollout_trig=0)
LIMIT_FIELDS = D.CFG_D[:11]
CONTROL = dict(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, trans_stopped_vel=0.01, rot_stopped_vel=0.01, prune_plan=1)
L0 = {k: CFG[k] for k in LIMIT_FIELDS}                                   # the fleet configuration's own
L1 = dict(L0, max_trans_vel=0.25, max_rot_vel=0.45)                       # MoveSlowAndClear's defaults (move_slow_and_clear.cpp:59-60)
L2 = dict(max_trans_vel=0.9, min_trans_vel=0.1, max_vel_x=0.9, min_vel_x=-0.2, max_vel_y=0.2, min_vel_y=-0.2, max_rot_vel=1.6,
          min_rot_vel=0.4, acc_lim_x=3.5, acc_lim_y=3.5, acc_lim_theta=4.5)  # faster in every velocity and acceleration: above the envelope
L3 = dict(L0, min_trans_vel=0.3, min_rot_vel=0.7)                         # the generator's minimum tests fire
CLASSES = (L0, L1, L2, L3)
# the scoring launches: the sweep's (T = 10 steps), the reference's default step rule, continued acceleration
VARIANTS = {
    "sweep": dict(),
    "by_distance": dict(discretize_by_time=0, sim_granularity=0.05),
    "rollout": dict(use_dwa=0),
}


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    assert hasattr(nav.lib(), "navgpu_planner_set_limits")
    return nav


def _record(lim, **control):
    return dict(lim, **dict(CONTROL, **control))


_SCENES = {}


def _scene(n_robots, size=SIZE, seed=0):
    """n_robots maps with lethal cells 0.4 - 0.9 m from the robot and a wall, a pose, a velocity and a plan per robot: even robots have
    plans long enough for bounded MapGrids under L0.  Computed once per shape and left unchanged."""
    key = (n_robots, size, seed)
    if key in _SCENES:
        return _SCENES[key]
    rs = np.random.RandomState(4200 + 17 * size + seed)
    masters, pos, vel, plans = [], [], [], []
    for i in range(n_robots):
        x, y, th = rs.uniform(0.8, 1.0), rs.uniform(1.3, size * D.RES - 1.3), rs.uniform(-0.25, 0.25)
        cells = np.zeros((size, size), np.uint8)
        for j in range(6):
            a, d = rs.uniform(0, 2 * np.pi), rs.uniform(0.4, 0.9) / D.RES
            cells[int(y / D.RES + d * np.sin(a)), int(x / D.RES + d * np.cos(a))] = D.LETHAL
        cells[8:size - 8, size - 4] = D.LETHAL
        m = D.inflate(cells)
        m.setflags(write=False)
        masters.append(m)
        pos.append(np.array([x, y, th], np.float32))
        vel.append(np.array([rs.uniform(0.2, 0.4), rs.uniform(-0.05, 0.05), rs.uniform(-0.3, 0.3)], np.float32))
        d = np.arange(0.0, 1.95 if i % 2 == 0 else 1.2, 0.05)
        heading = th + rs.uniform(-0.1, 0.1)
        plans.append(np.stack([x + d * np.cos(heading), y + d * np.sin(heading)], 1))
    _SCENES[key] = (masters, np.stack(pos), np.stack(vel), plans)
    return _SCENES[key]


def _fleet(nav, masters, cfg, max_sim_steps=32, size=SIZE, max_plan=MAX_PLAN):
    from navigation_amd import _lib as N
    fl = nav.Fleet(len(masters), size, size, D.RES, layers=N.LAYER_OBSTACLE, keep_sample_costs=True, max_sim_steps=max_sim_steps, max_plan=max_plan)
    fl.configure_planner(nav.DwaConfig(**cfg))
    fl.set_footprint(D.FP4)
    fl.upload(N.GRID_MASTER, np.stack(masters))
    fl.set_bounded_map_grids(1)
    return fl


def _set_classes(fl, classes):
    """robot i takes CLASSES[classes[i]] through set_limits, contiguous run by contiguous run of one class; L0 robots are left alone"""
    i = 0
    while i < len(classes):
        j = i
        while j < len(classes) and classes[j] == classes[i]:
            j += 1
        if classes[i] != 0:
            fl.set_limits([_record(CLASSES[classes[i]])] * (j - i), first=i)
        i = j


def _state(fl, i):
    """what a cycle leaves for robot i, as bytes - without the MapGrids, whose download completes a bounded search"""
    flags, prev = fl.oscillation(i, 1)
    return dict(result=bytes(fl.results(i, 1)[0]), trajectory=fl.trajectory(i).tobytes(), samples=b"".join(a.tobytes() for a in fl.samples(i)),
                oscillation=flags.tobytes() + prev.tobytes(), box=fl.wavefront_boxes(i, 1).tobytes())


def _grids(fl, i):
    from navigation_amd import _lib as N
    return [fl.download(g, i, 1)[0] for g in (N.GRID_PATH, N.GRID_GOAL, N.GRID_GOAL_FRONT)]


def _assert_same(a, b, what):
    for k in a:
        assert a[k] == b[k], (what, k)


def _assert_grids_same(fa, fb, i, what):
    x0, x1, y0, y1 = fa.wavefront_boxes(i, 1)[0]
    assert np.array_equal(fa.wavefront_boxes(i, 1), fb.wavefront_boxes(i, 1)), (what, "box")
    for ga, gb in zip(_grids(fa, i), _grids(fb, i)):
        assert np.array_equal(ga[y0:y1 + 1, x0:x1 + 1], gb[y0:y1 + 1, x0:x1 + 1]), (what, "MapGrid")


def _assert_oracle(fl, i, p, pos, vel, plan):
    """the bounds of tests/test_gpu_parity.py (_compare_cycle) for robot i against its own oracle planner"""
    o, _, _, cfull, ost = p.cycle(np.asarray(pos, np.float32), np.asarray(vel, np.float32), plan, np.asarray(D.FP4, np.float64))
    r = fl.results(i, 1)[0]
    cost, status, vels = fl.samples(i)
    assert np.array_equal(vels.view(np.uint32), p.samples().view(np.uint32)), "sample velocities differ"
    assert np.array_equal(status, ost)
    sc = status == 1
    assert np.array_equal(cost[sc] < 0, cfull[sc] < 0)
    assert np.array_equal(cost[sc][cost[sc] < 0], cfull[sc][cfull[sc] < 0]), "failure codes differ"
    assert np.allclose(cost[sc][cost[sc] >= 0], cfull[sc][cfull[sc] >= 0], rtol=0, atol=1e-5)
    assert (r.best_index, r.n_valid, r.n_scored) == (o.best_index, o.n_valid, o.n_scored)
    assert abs(r.cost - o.cost) <= 1e-5 and list(r.drive) == list(o.drive)
    return ost


def _advance(pos, vel, results, dt=0.2):
    """the robots move as commanded for dt (closed loop); a robot without a valid trajectory stands"""
    pos, vel = pos.copy(), vel.copy()
    for k, r in enumerate(results):
        c, th = r.drive, float(pos[k, 2])
        pos[k, 0] += np.float32((c[0] * np.cos(th) - c[1] * np.sin(th)) * dt)
        pos[k, 1] += np.float32((c[0] * np.sin(th) + c[1] * np.cos(th)) * dt)
        pos[k, 2] += np.float32(c[2] * dt)
        vel[k] = c[0], c[1], c[2]
    return pos, vel


def _sweep_scores(cfg):
    """the launch the configuration takes (planWindow): constant velocity, fixed step count, <= 127 steps, <= 8 vertices"""
    return bool(cfg["use_dwa"] and cfg["discretize_by_time"] and int(np.ceil(cfg["sim_time"] / cfg["sim_granularity"])) <= 127 and len(D.FP4) <= 8)


# ------------------------------------------------------------------------------------------------ 1. mixed against twins and oracle
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mixed_fleet_equals_twins_and_oracle(nav, orc, variant):
    classes = (0, 1, 2, 3, 1)
    cfg = dict(CFG, **VARIANTS[variant])
    assert _sweep_scores(cfg) == (variant == "sweep")
    masters, pos, vel, plans = _scene(len(classes))
    mixed = _fleet(nav, masters, cfg)
    twins = [_fleet(nav, masters, dict(cfg, **L)) for L in CLASSES]
    try:
        _set_classes(mixed, classes)
        assert [{k: r[k] for k in LIMIT_FIELDS} for r in mixed.limits()] == [CLASSES[c] for c in classes]
        oracles = [orc.DwaPlanner(masters[i], D.RES, 0.0, 0.0, orc.DwaConfig(**dict(cfg, **CLASSES[c]))) for i, c in enumerate(classes)]
        base = [orc.DwaPlanner(masters[i], D.RES, 0.0, 0.0, orc.DwaConfig(**cfg)) for i in range(len(classes))]  # every robot under L0
        for fl in [mixed] + twins:
            fl.set_plan()
        for p in oracles + base:
            p.set_plan()
        mixed.profile(True)
        mixed.profile_reset()
        fired = dict(min=0, max=0)
        for cyc in range(3):  # closed loop: the oscillation flags carry over, min_trans_vel enters updateOscillationFlags
            res = mixed.find_best_path(pos, vel, plans)
            for tw in twins:
                tw.find_best_path(pos, vel, plans)
            for i, c in enumerate(classes):
                _assert_same(_state(mixed, i), _state(twins[c], i), (variant, cyc, "robot", i, "class", c))
                st = _assert_oracle(mixed, i, oracles[i], pos[i], vel[i], plans[i])
                st0 = base[i].cycle(pos[i], vel[i], plans[i], np.asarray(D.FP4, np.float64))[4]
                # the reject tests tell the classes apart: slots of the same sample grid the generator rejects under one class only
                if c == 3 and len(st) == len(st0):
                    fired["min"] += int(((st == 0) & (st0 == 1)).sum())
                if c == 1 and len(st) == len(st0):
                    fired["max"] += int(((st == 0) & (st0 == 1)).sum())
            if cyc == 0:
                boxes = mixed.wavefront_boxes()
            pos, vel = _advance(pos, vel, res)
        assert fired["min"] > 0, "no slot rejected under L3 and accepted under L0"
        assert fired["max"] > 0, "no slot rejected under L1 and accepted under L0"
        assert mixed.profile_read()["k_score"][1] == 3  # one scoring launch per cycle: the sweep's where _sweep_scores says so
        for i, c in enumerate(classes):
            _assert_grids_same(mixed, twins[c], i, (variant, "robot", i))
        assert any(tuple(b) != (0, SIZE - 1, 0, SIZE - 1) for b in boxes), "no robot ran a bounded search"
        assert len({tuple(b[1::2] - b[0::2]) for b in boxes}) > 1, "every robot's box has the same extent: the reach does not follow the limits"
    finally:
        for fl in [mixed] + twins:
            fl.close()


# ------------------------------------------------------------------------------------------------ 2. a change between cycles
@pytest.mark.parametrize("in_flight", [1, 2])
def test_limits_change_between_cycles(nav, in_flight):
    masters, pos, vel, plans = _scene(4)
    cfg = dict(CFG)
    mixed, twin, plain = (_fleet(nav, masters, cfg) for _ in range(3))
    try:
        for fl in (mixed, twin, plain):
            fl.set_plan()
        twin.find_best_path(pos, vel, plans)
        first = plain.find_best_path(pos, vel, plans)
        pos2, vel2 = _advance(pos, vel, first)
        twin.configure_planner(nav.DwaConfig(**dict(cfg, **L1)))  # the twin was in the same state: cycle 1 on L0, then L1 fleet-wide
        twin.find_best_path(pos2, vel2, plans)
        plain.find_best_path(pos2, vel2, plans)
        mixed.set_cycles_in_flight(in_flight)
        mixed.stage_planner(pos, vel, plans)
        mixed.planner_cycle()
        if in_flight == 1:
            assert [bytes(r) for r in mixed.results()] == [bytes(r) for r in first]
        mixed.set_limits([_record(L1)], first=1)  # (two in flight: cycle 1 may still run)
        mixed.stage_planner(pos2, vel2, plans)
        mixed.planner_cycle()
        if in_flight == 2:
            prev = mixed.results_previous_into((nav.PlanResult * 4)())
            assert [bytes(r) for r in prev] == [bytes(r) for r in first], "cycle 1 did not run on L0"
        assert bytes(mixed.results(1, 1)[0]) != bytes(plain.results(1, 1)[0]), "L1 changes nothing for robot 1: the scene tells nothing"
        _assert_same(_state(mixed, 1), _state(twin, 1), ("robot 1 against its L1 twin", in_flight))
        for i in (0, 2, 3):
            _assert_same(_state(mixed, i), _state(plain, i), ("robot", i, "against the fleet nothing was set on", in_flight))
        mixed.set_cycles_in_flight(1)
        _assert_grids_same(mixed, twin, 1, "robot 1")
        for i in (0, 2, 3):
            _assert_grids_same(mixed, plain, i, ("robot", i))
    finally:
        for fl in (mixed, twin, plain):
            fl.close()


# ------------------------------------------------------------------------------------------------ 3. lists
def test_listed_cycle_with_mixed_limits(nav):
    classes = (3, 0, 1, 2)
    robots = [0, 2, 3]
    masters, pos, vel, plans = _scene(4)
    listed, ranged = _fleet(nav, masters, CFG), _fleet(nav, masters, CFG)
    try:
        for fl in (listed, ranged):
            fl.set_plan()
            fl.find_best_path(pos, vel, plans)  # every robot owns state, on L0
            _set_classes(fl, classes)
        before = _state(listed, 1)
        grids_before = _grids(listed, 1)
        _grids(ranged, 1)
        pos2, vel2 = _advance(pos, vel, listed.results())
        listed.stage_planner_list(robots, pos2[robots], vel2[robots], [plans[i] for i in robots])
        listed.planner_cycle_list(robots)
        got = listed.results_list(robots)
        ranged.stage_planner(pos2[0:1], vel2[0:1], plans[0:1], first=0)
        ranged.stage_planner(pos2[2:4], vel2[2:4], plans[2:4], first=2)
        ranged.planner_cycle(0, 1)
        ranged.planner_cycle(2, 2)
        for k, i in enumerate(robots):
            sb = _state(ranged, i)
            _assert_same(_state(listed, i), sb, ("robot", i))
            assert bytes(got[k]) == sb["result"]
        _assert_same(before, _state(listed, 1), "robot 1 was touched")
        for g0, g1 in zip(grids_before, _grids(listed, 1)):
            assert np.array_equal(g0, g1)
        # the listed robots ran on their own limits: their range twins of test 1's kind
        for i in robots:
            tw = _fleet(nav, masters, dict(CFG, **CLASSES[classes[i]]))
            try:
                tw.set_plan()
                tw.set_oscillation(*_osc_after_first(nav, masters, pos, vel, plans))
                tw.find_best_path(pos2, vel2, plans)
                assert bytes(tw.results(i, 1)[0]) == _state(listed, i)["result"], ("robot", i, "against its uniform twin")
            finally:
                tw.close()
    finally:
        listed.close()
        ranged.close()


_OSC = {}


def _osc_after_first(nav, masters, pos, vel, plans):
    """the oscillation state an L0 fleet holds after the first cycle of the scene (once)"""
    if "v" not in _OSC:
        fl = _fleet(nav, masters, CFG)
        try:
            fl.set_plan()
            fl.find_best_path(pos, vel, plans)
            _OSC["v"] = fl.oscillation()
        finally:
            fl.close()
    return _OSC["v"]


# ------------------------------------------------------------------------------------------------ 4. check_trajectories
def test_check_trajectories_reads_the_robots_own_limits(nav, orc):
    classes = (0, 1, 0, 1)
    masters, pos, vel, plans = _scene(4)
    mixed = _fleet(nav, masters, CFG)
    twins = {c: _fleet(nav, masters, dict(CFG, **CLASSES[c])) for c in (0, 1)}
    try:
        _set_classes(mixed, classes)
        for fl in [mixed] + list(twins.values()):
            fl.set_plan()
            fl.find_best_path(pos, vel, plans)
        # vmag between L1's and L0's max_trans_vel: the generator rejects it for an L1 robot - checkTrajectory then scores an empty
        # trajectory (dwa_planner.cpp:229-230), cost 0 - and rolls it out for an L0 robot
        probes = np.array([[0.4, 0.0, 0.1], [0.2, 0.0, -0.2], [0.5, 0.05, 0.0]], np.float32)
        ok, costs = mixed.check_trajectories(range(4), [probes] * 4)
        ok, costs = ok.reshape(4, -1), costs.reshape(4, -1)
        for i, c in enumerate(classes):
            tok, tcosts = twins[c].check_trajectories([i], [probes])
            assert np.array_equal(ok[i], tok) and costs[i].tobytes() == tcosts.tobytes(), ("robot", i, costs[i], tcosts)
            p = orc.DwaPlanner(masters[i], D.RES, 0.0, 0.0, orc.DwaConfig(**dict(CFG, **CLASSES[c])))
            p.set_plan()
            p.cycle(pos[i], vel[i], plans[i], np.asarray(D.FP4, np.float64), want_samples=False)
            assert list(ok[i]) == [p.check_trajectory(pos[i], vel[i], s) for s in probes], ("robot", i)
            if c == 1:
                assert costs[i][0] == 0.0 and costs[i][2] == 0.0 and ok[i][0], ("rejected probes score an empty trajectory", costs[i])
        assert any(costs[i][0] != 0.0 for i in (0, 2)), "the probe costs nothing for the L0 robots either: the scene tells nothing"
        # a probe right behind the change, no stage in between: the call itself carries the record up
        mixed.set_limits([_record(L1)], first=0)
        ok2, costs2 = mixed.check_trajectories([0], [probes])
        tok, tcosts = twins[1].check_trajectories([0], [probes])
        assert np.array_equal(ok2, tok) and costs2.tobytes() == tcosts.tobytes() and costs2[0] == 0.0
    finally:
        for fl in [mixed] + list(twins.values()):
            fl.close()


# ------------------------------------------------------------------------------------------------ 5. the control cycle
def _control_scenario():
    from navigation_amd import _lib as N
    goal = np.array([1.9, 1.6, 0.5])
    s = np.linspace(0.0, 1.6, 33)
    plan = np.stack([goal[0] - s[::-1] * np.cos(goal[2]), goal[1] - s[::-1] * np.sin(goal[2]), np.full_like(s, goal[2])], 1)
    slow = dict(L0, max_rot_vel=0.45, min_rot_vel=0.2)
    robots = [  # limits, control fields, offset from the goal along x, yaw offset, odometry, the branch wanted
        (L0, dict(), 0.03, -0.7, (0.3, 0.0, 0.2), N.BRANCH_STOP),
        (dict(L0, acc_lim_x=1.0, acc_lim_y=1.0, acc_lim_theta=1.5), dict(prune_plan=0), 0.03, -0.7, (0.3, 0.0, 0.2), N.BRANCH_STOP),
        (slow, dict(trans_stopped_vel=0.05, rot_stopped_vel=0.05), 0.03, -0.7, (0.03, 0.0, 0.02), N.BRANCH_ROTATE),  # stopped by its own measure only
        (L0, dict(xy_goal_tolerance=0.05), 0.1, -0.7, (0.2, 0.0, 0.0), N.BRANCH_DWA),     # outside its own tolerance, inside its neighbours'
        (L0, dict(yaw_goal_tolerance=0.3), 0.1, 0.2, (0.0, 0.0, 0.0), N.BRANCH_AT_GOAL),   # inside its own, 0.15 m, as robot 3 is not
    ]
    cells = np.zeros((SIZE, SIZE), np.uint8)
    cells[8:SIZE - 8, SIZE - 4] = D.LETHAL
    rs = np.random.RandomState(77)
    for _ in range(6):
        cells[rs.randint(4, 12), rs.randint(4, SIZE - 4)] = D.LETHAL
    master = D.inflate(cells)
    warm = np.array([goal[0] - 0.5 * np.cos(goal[2]), goal[1] - 0.5 * np.sin(goal[2]), goal[2]])
    pose = np.array([(goal[0] + dx, goal[1], goal[2] + dyaw) for _, _, dx, dyaw, _, _ in robots])
    vel = np.array([v for _, _, _, _, v, _ in robots], np.float64)
    return goal, plan, robots, master, warm, pose, vel


def test_control_cycle_reads_the_robots_own_limits(nav, orc):
    from navigation_amd import _lib as N
    from oracle import local_planner_oracle as lpo
    goal, plan, robots, master, warm, pose, vel = _control_scenario()
    n = len(robots)
    masters = [master] * n
    base_lim = dict(CONTROL, max_rot_vel=L0["max_rot_vel"], min_rot_vel=L0["min_rot_vel"], acc_lim_x=L0["acc_lim_x"], acc_lim_y=L0["acc_lim_y"],
                    acc_lim_theta=L0["acc_lim_theta"], sim_period=CFG["sim_period"], latch_xy_goal_tolerance=0)

    def local_limits(lim, control):
        return dict(base_lim, **dict({k: lim[k] for k in ("max_rot_vel", "min_rot_vel", "acc_lim_x", "acc_lim_y", "acc_lim_theta")}, **control))

    mixed = _fleet(nav, masters, CFG)
    twins, oracles = [], []
    try:
        mixed.configure_local_planner(**base_lim)
        for i, (lim, control, *_r) in enumerate(robots):
            mixed.set_limits([_record(lim, **control)], first=i)
            tw = _fleet(nav, masters, dict(CFG, **lim))
            tw.configure_local_planner(**local_limits(lim, control))
            twins.append(tw)
            o = lpo.DwaPlannerRos(orc.DwaPlanner(master, D.RES, 0.0, 0.0, orc.DwaConfig(**dict(CFG, **lim))), local_limits(lim, control), SIZE, SIZE,
                                  D.RES, D.FP4)
            o.set_plan(plan, None)
            oracles.append(o)
        for fl in [mixed] + twins:
            for i in range(n):
                fl.set_global_plan(i, plan, None)
        for cyc in range(3):  # a warm-up half a metre short of the goal (DWA: the MapGrids checkTrajectory reads), then two cycles
            p = np.stack([warm] * n) if cyc == 0 else pose
            v = np.tile([0.2, 0.0, 0.0], (n, 1)) if cyc == 0 else vel
            got = mixed.compute_velocity_commands(p, v)
            for i in range(n):
                t = twins[i].compute_velocity_commands(p, v)[i]
                assert bytes(got[i]) == bytes(t), (cyc, "robot", i, tuple(got[i].cmd_vel), got[i].branch, tuple(t.cmd_vel), t.branch)
                want = oracles[i].compute_velocity_commands(p[i], v[i])
                g = got[i]
                assert bool(g.ok) == bool(want["ok"]) and g.branch == want["branch"], (cyc, i, g.ok, g.branch, want)
                assert tuple(g.cmd_vel) == tuple(float(x) for x in want["cmd"]), (cyc, i, tuple(g.cmd_vel), want["cmd"])
                assert g.local_plan_points == want["local_plan_points"] and g.trajectory_points == want["trajectory_points"], (cyc, i)
            if cyc == 0:
                assert all(g.branch == N.BRANCH_DWA for g in got)
            if cyc == 1:
                assert [g.branch for g in got] == [r[5] for r in robots]
                assert tuple(got[0].cmd_vel) != tuple(got[1].cmd_vel), "stopWithAccLimits: the acceleration limits tell nothing"
                assert abs(got[2].cmd_vel[2]) <= 0.45, "rotateToGoal above the robot's max_rot_vel"
                assert got[0].local_plan_points != got[1].local_plan_points, "prune_plan on / off tells nothing"
            if cyc >= 1:
                for i in range(n):
                    c, th = got[i].cmd_vel, pose[i, 2]
                    pose[i, 0] += (c[0] * np.cos(th) - c[1] * np.sin(th)) * CFG["sim_period"]
                    pose[i, 1] += (c[0] * np.sin(th) + c[1] * np.cos(th)) * CFG["sim_period"]
                    pose[i, 2] += c[2] * CFG["sim_period"]
                    vel[i] = tuple(c)
        reached = mixed.is_goal_reached(pose, vel)
        for i in range(n):
            assert reached[i] == twins[i].is_goal_reached(pose, vel)[i] == oracles[i].is_goal_reached(pose[i], vel[i]), ("is_goal_reached", i)
    finally:
        for fl in [mixed] + twins:
            fl.close()


# ------------------------------------------------------------------------------------------------ 6. trajectory cloud
@pytest.mark.parametrize("variant", ["sweep", "rollout"])
def test_trajectory_cloud_of_a_limited_robot(nav, variant):
    classes = (0, 3, 1)
    cfg = dict(CFG, **VARIANTS[variant])
    masters, pos, vel, plans = _scene(3)
    mixed, twin = _fleet(nav, masters, cfg), _fleet(nav, masters, dict(cfg, **L3))
    try:
        _set_classes(mixed, classes)
        for fl in (mixed, twin):
            fl.set_plan()
            fl.set_trajectory_cloud(True, first=1, count=1)
            fl.find_best_path(pos, vel, plans)
        a, b = mixed.sample_terms(1), twin.sample_terms(1)
        assert a.tobytes() == b.tobytes()
        assert (a["status"] == 0).any() and (a["status"] == 1).any(), "L3 rejects nothing or everything: the scene tells nothing"
        for ref in (True, False):
            ca, cb = mixed.trajectory_cloud(1, ref), twin.trajectory_cloud(1, ref)
            assert len(ca) > 0 and ca.tobytes() == cb.tobytes()
    finally:
        mixed.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 7. round trip, resets, errors
def test_round_trip_and_fleet_wide_reset(nav):
    masters, pos, vel, plans = _scene(4)
    fl = _fleet(nav, masters, CFG)
    try:
        recs = [_record(L1, xy_goal_tolerance=0.2), _record(L3, prune_plan=0, rot_stopped_vel=0.03)]
        fl.set_limits(recs, first=1)
        got = fl.limits()
        assert got[1] == recs[0] and got[2] == recs[1]
        assert {k: got[0][k] for k in LIMIT_FIELDS} == L0 and {k: got[3][k] for k in LIMIT_FIELDS} == L0
        arr = np.zeros(1, [(k, np.float64) for k in recs[0] if k != "prune_plan"] + [("prune_plan", np.int32)])
        for k, v in recs[1].items():
            arr[k] = v
        fl.set_limits(arr, first=3)  # a structured array
        assert fl.limits(3, 1)[0] == recs[1]
        fl.configure_local_planner(**dict(CONTROL, max_rot_vel=1.0, min_rot_vel=0.4, acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2, sim_period=0.05,
                                          latch_xy_goal_tolerance=0, xy_goal_tolerance=0.11))
        got = fl.limits()
        assert all(r["xy_goal_tolerance"] == 0.11 and r["prune_plan"] == 1 for r in got)
        assert {k: got[1][k] for k in LIMIT_FIELDS} == L1  # the planner's half stays the robot's
        fl.configure_planner(nav.DwaConfig(**dict(CFG, max_vel_x=0.5)))
        assert all({k: r[k] for k in LIMIT_FIELDS} == dict(L0, max_vel_x=0.5) for r in fl.limits())
    finally:
        fl.close()


def test_invalid_input_changes_nothing(nav):
    masters, pos, vel, plans = _scene(4)
    fl, plain = _fleet(nav, masters, CFG), _fleet(nav, masters, CFG)
    L = nav.lib()
    try:
        for f in (fl, plain):
            f.set_plan()
        rec = (nav._lib.RobotLimits * 2)()
        for r in rec:
            for k, v in _record(L1).items():
                setattr(r, k, v)
        p = C.cast(rec, C.c_void_p)
        before = fl.limits()
        assert L.navgpu_planner_set_limits(fl.h, 3, 2, p) == NAVGPU_ERR_INVALID  # past the fleet's end
        assert L.navgpu_planner_set_limits(fl.h, 4, 1, p) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_set_limits(fl.h, 0, 0, p) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_set_limits(fl.h, 0, 1, None) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_get_limits(fl.h, 0, 1, None) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_get_limits(fl.h, 2, 3, p) == NAVGPU_ERR_INVALID
        for bad in (float("nan"), float("inf")):
            for field in ("max_trans_vel", "acc_lim_theta", "rot_stopped_vel"):
                setattr(rec[1], field, bad)
                assert L.navgpu_planner_set_limits(fl.h, 0, 2, p) == NAVGPU_ERR_INVALID, (field, bad)  # the good record in front changes nothing either
                setattr(rec[1], field, _record(L1)[field])
        assert fl.limits() == before
        a, b = fl.find_best_path(pos, vel, plans), plain.find_best_path(pos, vel, plans)
        assert [bytes(r) for r in a] == [bytes(r) for r in b]
        for i in range(4):
            _assert_same(_state(fl, i), _state(plain, i), ("robot", i))
    finally:
        fl.close()
        plain.close()


def test_step_capacity_is_checked_and_the_limits_stay(nav):
    cfg = dict(CFG, **VARIANTS["by_distance"])
    masters, pos, vel, plans = _scene(4)
    # discretize_by_time = 0: L0 needs ceil(0.5501 / 0.05) + 1 = 13 steps, L2 ceil(0.9001 / 0.05) + 1 = 20
    fl, twin = _fleet(nav, masters, cfg, max_sim_steps=14), _fleet(nav, masters, cfg, max_sim_steps=14)
    try:
        for f in (fl, twin):
            f.set_plan()
        rec = (nav._lib.RobotLimits * 1)()
        for k, v in _record(L2).items():
            setattr(rec[0], k, v)
        assert nav.lib().navgpu_planner_set_limits(fl.h, 2, 1, C.cast(rec, C.c_void_p)) == NAVGPU_ERR_CAPACITY
        assert {k: fl.limits(2, 1)[0][k] for k in LIMIT_FIELDS} == L0
        fl.find_best_path(pos, vel, plans)
        twin.find_best_path(pos, vel, plans)
        for i in range(4):
            _assert_same(_state(fl, i), _state(twin, i), ("robot", i))
    finally:
        fl.close()
        twin.close()


def test_failed_image_growth_leaves_the_limits_in_force(nav):
    masters, pos, vel, plans = _scene(4)
    fl, twin0, twin2 = _fleet(nav, masters, CFG), _fleet(nav, masters, CFG), _fleet(nav, masters, dict(CFG, **L2))
    try:
        for f in (fl, twin0, twin2):
            f.set_plan()
        rec = (nav._lib.RobotLimits * 1)()
        for k, v in _record(L2).items():
            setattr(rec[0], k, v)
        fl.set_alloc_limit(1024)  # the image of a window planned for L2's 0.9 m/s is larger than the one in place
        assert nav.lib().navgpu_planner_set_limits(fl.h, 2, 1, C.cast(rec, C.c_void_p)) == NAVGPU_ERR_HIP
        assert {k: fl.limits(2, 1)[0][k] for k in LIMIT_FIELDS} == L0
        first = fl.find_best_path(pos, vel, plans)
        twin0.find_best_path(pos, vel, plans)
        for i in range(4):
            _assert_same(_state(fl, i), _state(twin0, i), ("robot", i, "after the failed call"))
        fl.set_alloc_limit(0)
        fl.set_limits([_record(L2)], first=2)
        pos2, vel2 = _advance(pos, vel, first)
        twin2.set_oscillation(*twin0.oscillation())
        fl.find_best_path(pos2, vel2, plans)
        twin2.find_best_path(pos2, vel2, plans)
        twin0.find_best_path(pos2, vel2, plans)
        _assert_same(_state(fl, 2), _state(twin2, 2), "robot 2 against its L2 twin")
        assert _state(fl, 2)["samples"] != _state(twin0, 2)["samples"]
        for i in (0, 1, 3):
            _assert_same(_state(fl, i), _state(twin0, i), ("robot", i))
    finally:
        for f in (fl, twin0, twin2):
            f.close()


# ------------------------------------------------------------------------------------------------ 8. one larger shape
def test_larger_shape(nav):
    """400 x 400, 32 x 32 x 16 samples, six robots in three interleaved classes: the sweep's row groups and the bounded wavefront boxes
    differ per robot at this size"""
    size, classes = 400, (0, 1, 2, 0, 1, 2)
    cfg = dict(CFG, vx_samples=32, vy_samples=32, vth_samples=16, sim_time=1.7, sim_granularity=0.17)
    rs = np.random.RandomState(8)
    masters, pos, vel, plans = [], [], [], []
    for i in range(len(classes)):
        x, y, th = rs.uniform(4.0, 6.0), rs.uniform(4.0, 16.0), rs.uniform(-0.3, 0.3)
        cells = np.zeros((size, size), np.uint8)
        for j in range(12):
            a, d = rs.uniform(0, 2 * np.pi), rs.uniform(0.4, 1.5) / D.RES
            cells[int(y / D.RES + d * np.sin(a)), int(x / D.RES + d * np.cos(a))] = D.LETHAL
        cells[20:size - 20, size - 20] = D.LETHAL
        masters.append(D.inflate(cells))
        pos.append(np.array([x, y, th], np.float32))
        vel.append(np.array([rs.uniform(0.2, 0.4), 0.0, rs.uniform(-0.3, 0.3)], np.float32))
        d = np.arange(0.0, 9.0, 0.05)
        plans.append(np.stack([x + d * np.cos(th), y + d * np.sin(th)], 1))
    pos, vel = np.stack(pos), np.stack(vel)

    def fleet(c):
        return _fleet(nav, masters, c, max_sim_steps=16, size=size, max_plan=256)

    mixed = fleet(cfg)
    twins = [fleet(dict(cfg, **CLASSES[c])) for c in (0, 1, 2)]
    try:
        _set_classes(mixed, classes)
        for fl in [mixed] + twins:
            fl.set_plan()
            fl.find_best_path(pos, vel, plans)
        for i, c in enumerate(classes):
            _assert_same(_state(mixed, i), _state(twins[c], i), ("robot", i, "class", c))
        res = mixed.results()
        assert any(r.cost >= 0 for r in res)
        boxes = mixed.wavefront_boxes()
        assert len({tuple(b[1::2] - b[0::2]) for b in boxes}) >= 2 and all(tuple(b) != (0, size - 1, 0, size - 1) for b in boxes), boxes
    finally:
        for fl in [mixed] + twins:
            fl.close()
