"""The TrajectoryPlannerROS mirror for a fleet (navgpu_tp_ros_*).  Need a real MI355X.

TrajectoryPlannerROS needs tf and ROS and cannot be compiled against the reference tree, so no fixture pins this row.  The expectation has
two halves: the branch logic, the latch and the flags come from the Python restatement of trajectory_planner_ros.cpp in
tests/tp_ros_ref.py; everything the device answers comes from a TWIN FLEET driven by hand, robot by robot, through the single entry
points that have their own pinned tests (navgpu_local_plan_window, tp_update_plan, tp_find_best_path, tp_score_trajectory)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tp_ros_ref as R  # noqa: E402
from tp_reference_cases import FP4, FP_WIDE, LETHAL, RES  # noqa: E402

pytestmark = pytest.mark.gpu

NX = NY = 64
MAX_PLAN, STEPS = 256, 96
THRESHOLD = max(NX * RES / 2.0, NY * RES / 2.0)  # transformGlobalPlan's reach (goal_functions.cpp:118-119)
CFG = dict(sim_time=1.7, sim_granularity=0.025, angular_sim_granularity=0.025, vx_samples=4, vtheta_samples=5)
PARAMS = dict(xy_goal_tolerance=0.10, yaw_goal_tolerance=0.05, rot_stopped_velocity=1e-2, trans_stopped_velocity=1e-2,
              latch_xy_goal_tolerance=1, prune_plan=1)


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _window(L):
    """navgpu_local_plan_window as tp_ros_ref.decide's window function"""
    def window(plan, pose, T, prune):
        p = np.ascontiguousarray(plan, np.float64).reshape(-1, 3)
        pose = np.ascontiguousarray(pose, np.float64)
        t = None if T is None else np.ascontiguousarray(T, np.float64)
        out = np.zeros((MAX_PLAN, 3))
        n_out, n_erased = C.c_uint32(), C.c_uint32()
        rc = L.navgpu_local_plan_window(_p(p), len(p), _p(pose), None if t is None else _p(t), THRESHOLD, int(prune), _p(out), MAX_PLAN,
                                        C.byref(n_out), C.byref(n_erased))
        assert rc == 0, rc
        return [tuple(float(v) for v in row) for row in out[:n_out.value]], n_erased.value
    return window


def _plan(p0, p1, yaw, step=0.05, yaw_step=0.0):
    """(x, y, yaw) poses every `step` metres from p0 to p1; pose i has yaw + i * yaw_step"""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    n = max(1, int(round(float(np.hypot(*(p1 - p0))) / step)))
    return np.array([[*(p0 + (p1 - p0) * (k / n)), yaw + k * yaw_step] for k in range(n + 1)])


def _fleet(nav, n, maps, wide=()):
    from navigation_amd import _lib as N
    fl = nav.Fleet(n, NX, NY, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=STEPS, max_plan=MAX_PLAN)
    fl.set_origin(np.zeros((n, 2)))
    fl.upload(N.GRID_MASTER, np.stack(maps))
    fl.set_footprint(np.asarray(FP4, np.float64))
    for i in wide:
        fl.set_footprint(np.asarray(FP_WIDE, np.float64), first=i, count=1)
    fl.configure_trajectory_planner(N.TpConfig(**CFG))
    return fl


def _cycle(fl, twin, ref, cfg, poses, vels, have, window, what):
    """one navgpu_tp_ros_compute_velocity_commands over the whole fleet against tp_ros_ref.decide + the twin driven by hand"""
    from navigation_amd import _lib as N
    before = [fl.download(g) for g in (N.GRID_PATH, N.GRID_GOAL)]
    got = fl.tp_ros_compute_velocity_commands(poses, vels, have_pose=have)
    dec = R.decide(ref, PARAMS, cfg, [tuple(p) for p in poses], [tuple(v) for v in vels], have, window)
    after = [fl.download(g) for g in (N.GRID_PATH, N.GRID_GOAL)]
    pos32, vel32 = np.asarray(poses, np.float32), np.asarray(vels, np.float32)
    for i, d in enumerate(dec):
        where = f"{what} robot {i} kind {d.kind}"
        g = got[i]
        want_cmd, want_ok, want_points = (0.0, 0.0, 0.0), 0, 0
        if d.kind in (R.ROLLOUT, R.REACHED):  # updatePlan(transformed_plan) + findBestPath, also where the result is discarded
            twin.tp_update_plan(i, np.asarray(d.window)[:, :2], compute_dists=False)
            r = twin.tp_find_best_path(pos32[i:i + 1], vel32[i:i + 1], first=i)[0]
            assert fl.tp_samples(i) == twin.tp_samples(i), where
            assert np.array_equal(fl.tp_trajectory(i), twin.tp_trajectory(i)), where
            assert bytes(fl.tp_state(i, 1)[0]) == bytes(twin.tp_state(i, 1)[0]), where
            for k, gid in enumerate((N.GRID_PATH, N.GRID_GOAL)):  # this cycle's grids
                assert np.array_equal(after[k][i], twin.download(gid, i, 1)[0]), (where, gid)
            if d.kind == R.ROLLOUT:
                want_cmd, want_ok = tuple(r.drive), int(r.cost >= 0)
                want_points = r.n_points if want_ok else 0
        else:  # no updatePlan / findBestPath: the grids are the ones the cycle found
            for k in range(2):
                assert np.array_equal(after[k][i], before[k][i]), where
        if d.kind == R.REACHED:  # the candidate against this cycle's grids
            cost = twin.tp_score_trajectory(i, poses[i], vels[i], d.candidate)
            want_ok = int(cost >= 0)
            want_cmd = d.candidate if want_ok else (0.0, 0.0, 0.0)
        if d.kind == R.AT_GOAL:
            want_ok = 1
        print(f"{where}: branch {g.branch} ok {g.ok} cmd {tuple(g.cmd_vel)} window {g.local_plan_points} points {g.trajectory_points}")
        assert g.branch == d.branch, (where, g.branch, d.branch)
        assert g.ok == want_ok and tuple(g.cmd_vel) == tuple(want_cmd), (where, g.ok, want_ok, tuple(g.cmd_vel), want_cmd)
        assert g.local_plan_points == len(d.window) and g.trajectory_points == want_points, (where, g.local_plan_points, len(d.window))
        assert np.array_equal(fl.tp_ros_transformed_plan(i), np.asarray(d.window, np.float64).reshape(-1, 3)), where
        assert np.array_equal(fl.tp_ros_global_plan(i), np.asarray(ref[i].plan, np.float64).reshape(-1, 3)), where  # pruned in lockstep
    assert fl.tp_ros_is_goal_reached() == [r.reached for r in ref], what
    return got, dec, (before, after)


def test_control_cycle_of_eight(nav):
    from navigation_amd import _lib as N
    L = nav.lib()
    window = _window(L)
    maps = [np.zeros((NY, NX), np.uint8) for _ in range(8)]
    maps[4][:, 28] = LETHAL  # a corridor 0.35 m wide round x = 1.625: the wide robot stands across it and cannot turn
    maps[4][:, 36] = LETHAL
    fl, twin = _fleet(nav, 8, maps, wide=(4,)), _fleet(nav, 8, maps, wide=(4,))
    try:
        cfg = N.TpConfig(**CFG)
        fl.configure_tp_ros(**PARAMS)
        long_plan = _plan((0.3, 0.3), (2.7, 2.7), 0.0, yaw_step=0.01)  # every pose its own yaw: which pose is the goal shows
        short = _plan((0.5, 2.0), (1.5, 2.0), 0.0)
        plans = [_plan((0.5, 1.6), (2.9, 1.6), 0.0),       # 0 drives
                 long_plan,                                 # 1 at the end of a long plan, still moving: stop
                 short,                                     # 2 at the end, standing, facing elsewhere: rotate
                 short,                                     # 3 at the end, facing the goal's way: at goal
                 _plan((1.625, 0.8), (1.625, 1.6), 0.9),    # 4 wide robot in the corridor, has to turn by 0.9: blocked
                 short,                                     # 5 has no pose
                 np.zeros((0, 3)),                          # 6 has an empty plan
                 _plan((2.6, 2.6), (3.0, 3.0), 0.0)]        # 7 stands out of reach of its plan
        fl.tp_ros_set_plans(plans)
        ref = [R.Robot() for _ in range(8)]
        for r, p in zip(ref, plans):
            r.set_plan(p)
        # grids from an older plan on every robot: a cycle that leaves a robot's grids alone leaves these
        old = [_plan((0.4, 0.4), (1.0, 0.4), 0.0)[:, :2]] * 8
        fl.tp_update_plans(old, compute_dists=True)
        for i in range(8):
            twin.tp_update_plan(i, old[i], compute_dists=True)
        end = long_plan[-1]
        poses = np.array([(0.5, 1.6, 0.0), (end[0] - 0.02, end[1] - 0.02, 0.8), (1.47, 2.0, 0.9), (1.47, 2.0, 0.02), (1.625, 1.58, 0.0), (1.0, 2.0, 0.0),
                          (1.0, 1.0, 0.0), (0.3, 0.3, 0.0)])
        vels = np.array([(0.2, 0.0, 0.0), (0.3, 0.0, 0.2), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0),
                         (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
        have = [True, True, True, True, True, False, True, True]
        got, dec, (before, after) = _cycle(fl, twin, ref, cfg, poses, vels, have, window, "cycle 1")
        assert [g.branch for g in got] == [N.BRANCH_ROLLOUT, N.BRANCH_STOP, N.BRANCH_ROTATE, N.BRANCH_AT_GOAL, N.BRANCH_ROTATE, N.BRANCH_NONE,
                                           N.BRANCH_NONE, N.BRANCH_NONE]
        assert [g.ok for g in got] == [1, 1, 1, 1, 0, 0, 0, 0], [g.ok for g in got]
        assert got[0].trajectory_points > 0 and got[0].cmd_vel[0] > 0
        assert tuple(got[4].cmd_vel) == (0.0, 0.0, 0.0) and dec[4].candidate[2] > 0  # the turn was asked for, and refused
        assert got[7].local_plan_points == 0 and got[6].local_plan_points == 0
        for k in range(2):  # reached-position robots: refreshed; the robot at its goal: not
            assert not np.array_equal(after[k][1], before[k][1]) and not np.array_equal(after[k][2], before[k][2])
            assert np.array_equal(after[k][3], before[k][3])
        assert fl.tp_ros_is_goal_reached() == [False, False, False, True, False, False, False, False]
        assert [r.latch for r in ref] == [False, True, True, False, True, False, False, False]

        # cycle 2: robot 0 has driven on (pruning); robot 1, latched, is put back near the start of its plan: its window ends about 1 m
        # before the global goal, and the window's last pose is the goal - it still stops; robot 2 has drifted 0.3 m out of tolerance
        # and keeps rotating on the latch
        poses[0] = (1.8, 1.6, 0.0)
        poses[1] = (0.5, 0.5, 1.0)
        poses[2] = (1.2, 2.05, 0.9)
        n0 = len(ref[0].plan)
        got, dec, _ = _cycle(fl, twin, ref, cfg, poses, vels, have, window, "cycle 2")
        assert len(ref[0].plan) < n0 and got[0].branch == N.BRANCH_ROLLOUT  # poses more than 1 m behind the robot were erased
        assert got[1].branch == N.BRANCH_STOP and got[1].ok == 1
        assert math.hypot(dec[1].window[-1][0] - end[0], dec[1].window[-1][1] - end[1]) > 0.9 and dec[1].goal_th != end[2]
        assert got[2].branch == N.BRANCH_ROTATE and math.hypot(poses[2][0] - 1.5, poses[2][1] - 2.0) > 0.3

        # a new plan clears the latch and the reached flag, not rotating_to_goal_
        fl.tp_ros_set_plans([short, short], first=2)
        ref[2].set_plan(short)
        ref[3].set_plan(short)
        assert fl.tp_ros_is_goal_reached() == [False] * 8
        got, dec, _ = _cycle(fl, twin, ref, cfg, poses, vels, have, window, "cycle 3")
        assert got[2].branch == N.BRANCH_ROLLOUT and got[3].branch == N.BRANCH_AT_GOAL and ref[2].rotating
        assert fl.tp_ros_is_goal_reached()[3]

        # cycle 4: robot 2 is back in tolerance and moving - it was rotating before, so it rotates (it does not stop first)
        poses[2] = (1.47, 2.0, 0.9)
        vels[2] = (0.3, 0.0, 0.0)
        got, dec, _ = _cycle(fl, twin, ref, cfg, poses, vels, have, window, "cycle 4")
        assert got[2].branch == N.BRANCH_ROTATE and got[1].branch == N.BRANCH_STOP
    finally:
        fl.close()
        twin.close()


def test_window_longer_than_max_plan_is_a_capacity_error(nav):
    from navigation_amd import _lib as N
    fl = _fleet(nav, 1, [np.zeros((NY, NX), np.uint8)])
    try:
        fl.configure_tp_ros(**PARAMS)
        fl.tp_ros_set_plans([_plan((0.5, 1.6), (2.0, 1.6), 0.0, step=0.005)])  # 301 poses within reach
        with pytest.raises(N.NavgpuError, match=r"\(-4\)"):
            fl.tp_ros_compute_velocity_commands([(0.5, 1.6, 0.0)], [(0.0, 0.0, 0.0)])
    finally:
        fl.close()


@pytest.mark.parametrize("update_map", [False, True])
def test_check_trajectories(nav, update_map):
    """scoreTrajectory / checkTrajectory(vx, vy, vtheta, update_map) for robots 0, 1, 3 of 4 (1 has no pose) against the twin's
    tp_update_plan([pose], True) + tp_score_trajectory"""
    from navigation_amd import _lib as N
    maps = [np.zeros((NY, NX), np.uint8) for _ in range(4)]
    maps[3][:, 40] = LETHAL
    fl, twin = _fleet(nav, 4, maps), _fleet(nav, 4, maps)
    try:
        fl.configure_tp_ros(**PARAMS)
        plan = _plan((0.5, 1.6), (1.9, 1.6), 0.0)[:, :2]
        fl.tp_update_plans([plan] * 4, compute_dists=True)
        for i in range(4):
            twin.tp_update_plan(i, plan, compute_dists=True)
        inst = [0, 1, 3]
        poses = np.array([(0.62, 1.62, 0.1), (0.7, 1.5, 0.0), (1.2, 1.62, 0.0)])
        vels = np.array([(0.2, 0.0, 0.1), (0.0, 0.0, 0.0), (0.5, 0.0, 0.0)])
        samples = [np.array([(0.3, 0.0, 0.2), (0.0, 0.0, -0.8)]), np.array([(0.1, 0.0, 0.0)]), np.array([(0.55, 0.0, 0.0), (0.0, 0.0, 0.5), (-0.1, 0.0, 0.0)])]
        costs, ok = fl.tp_ros_check_trajectories(inst, poses, vels, samples, update_map=update_map, have_pose=[True, False, True])
        want = []
        for i, pose, vel, run, have in zip(inst, poses, vels, samples, (True, False, True)):
            if have and update_map:
                twin.tp_update_plan(i, pose[None, :2], compute_dists=True)
            want += [twin.tp_score_trajectory(i, pose, vel, s) if have else -1.0 for s in run]
        print(f"update_map {update_map}: costs {costs.tolist()} twin {want}")
        assert costs.tolist() == want and ok.tolist() == [w >= 0 for w in want]
        assert costs[2] == -1.0 and costs[3] == -1.0 and costs[0] >= 0  # no pose; robot 3 drives into its wall
        for gid in (N.GRID_PATH, N.GRID_GOAL):  # with update_map the planner's plan is the robot's pose: its grids say so
            assert np.array_equal(fl.download(gid), twin.download(gid)), gid
        if update_map:
            goal = fl.download(N.GRID_GOAL, 0, 1)[0]
            assert goal[int(1.62 / RES), int(0.62 / RES)] == 0  # the goal is the robot's own cell
        # the next findBestPath plans on what updatePlan left
        pos, vel = np.tile(np.asarray((0.6, 1.6, 0.0), np.float32), (4, 1)), np.zeros((4, 3), np.float32)
        assert [bytes(x) for x in fl.tp_find_best_path(pos, vel)] == [bytes(x) for x in twin.tp_find_best_path(pos, vel)]
    finally:
        fl.close()
        twin.close()
