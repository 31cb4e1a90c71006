"""The legacy TrajectoryPlanner for a robot list (navgpu_tp_update_plans_list / navgpu_tp_find_best_path_list), the TrajectoryPlannerROS
control cycle and checkTrajectory(update_map) that use them, and the listed completion of bounded MapGrids.  Need a real MI355X.

No robot's data depends on another's, so the bar is bit equality throughout: a fleet driven through the listed calls against a twin
driven through the range calls, contiguous run by contiguous run; and, for the robots outside the list, the fleet against itself before
the listed calls.  The control cycle is held against tests/tp_ros_ref.py and a twin driven by hand, as tests/test_gpu_tp_ros.py holds it,
and its launches are counted: one wavefront bracket and one rollout bracket per call however the robots lie (the stop / rotate
candidates' k_tp_probe launch is bracketed under k_score as well: one more where a robot has reached its position)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tp_ros_ref as R  # noqa: E402
from tp_reference_cases import FP4, FP_WIDE, LETHAL, RES  # noqa: E402
from test_gpu_tp_ros import CFG, PARAMS, _cycle, _fleet as _ros_fleet, _plan, _window  # noqa: E402

pytestmark = pytest.mark.gpu

NAVGPU_ERR_INVALID, NAVGPU_ERR_CAPACITY, NAVGPU_ERR_STATE = -1, -4, -5
TP_ESCAPING = 1 << 8
N_ROBOTS, MAX_PLAN, STEPS = 8, 256, 96
LIST = (0, 2, 3, 7)
# what the parity test is parametrised over; wide: the listed robot 3 has the wide footprint (else the unlisted robot 5 has it)
VARIANTS = {
    "holonomic": dict(cfg=dict(holonomic_robot=1)),
    "non_holonomic": dict(cfg=dict(holonomic_robot=0)),
    "dwa": dict(cfg=dict(dwa=1)),
    "heading_scoring": dict(cfg=dict(heading_scoring=1)),
    "escape": dict(boxed=0),          # the listed robot 0 stands on a lethal cell: every rollout fails, it backs up and escapes
    "empty_plan": dict(empty=2),      # the listed robot 2 has no plan
    "wide_listed": dict(wide=(3,)),   # within-cell counts differ inside one packed block; the first call grows the cell capacity
}


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _runs(robots):
    """the contiguous runs (first, count) of a strictly increasing list"""
    runs = []
    for r in robots:
        if runs and runs[-1][0] + runs[-1][1] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    return [tuple(r) for r in runs]


_SCENES = {}


def _scene(n, nx, ny):
    """n maps with a few lethal cells beside the robots' plans, an older plan per robot, and two cycles of (pose, velocity, plan) per
    robot.  The robots stand in the first 64 columns whatever the width.  Computed once per shape and left unchanged."""
    if (n, nx, ny) in _SCENES:
        return _SCENES[(n, nx, ny)]
    rs = np.random.RandomState(77 + nx)
    maps, old, cycles = [], [], [[], []]
    for i in range(n):
        x, y, th = 0.6 + 0.04 * i, 0.9 + (ny * RES - 1.8) * i / max(n - 1, 1), 0.1 * i - 0.3
        m = np.zeros((ny, nx), np.uint8)
        for j in range(5):
            m[int(y / RES) + rs.randint(5, 9) * (1 if j % 2 else -1), int(x / RES) + rs.randint(8, 30)] = LETHAL
        m.setflags(write=False)
        maps.append(m)
        old.append(_plan((0.4, 0.4), (1.0, 0.4), 0.0)[:, :2])
        for c in range(2):
            pos = np.array([x + 0.05 * c, y + 0.01 * c, th + 0.03 * c], np.float32)
            vel = np.array([0.2 + 0.02 * i, 0.0, 0.1 - 0.05 * c], np.float32)
            plan = _plan((float(pos[0]), float(pos[1])), (2.0 + 0.1 * i, y + 0.2 * (c + 1) * (-1) ** i), 0.0)[:, :2]
            cycles[c].append((pos, vel, plan))
    _SCENES[(n, nx, ny)] = (maps, old, cycles)
    return _SCENES[(n, nx, ny)]


def _fleet(nav, nx, ny, maps, wide=(5,), cfg=None):
    from navigation_amd import _lib as N
    n = len(maps)
    fl = nav.Fleet(n, nx, ny, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=STEPS, max_plan=MAX_PLAN)
    fl.set_origin(np.zeros((n, 2)))
    fl.upload(N.GRID_MASTER, np.stack(maps))
    fl.set_footprint(np.asarray(FP4, np.float64))
    for i in wide:
        if i < n:
            fl.set_footprint(np.asarray(FP_WIDE, np.float64), first=i, count=1)
    if cfg is not None:
        fl.configure_trajectory_planner(N.TpConfig(**dict(CFG, **cfg)))
    return fl


def _grids(fl, i):
    from navigation_amd import _lib as N
    return [fl.download(g, i, 1)[0] for g in (N.GRID_PATH, N.GRID_GOAL)]


def _state(fl, i):
    """what the legacy planner holds for robot i, as bytes: the calls of the last cycle, the winner's points, the persistent state, both grids"""
    return dict(samples=repr(fl.tp_samples(i)), trajectory=fl.tp_trajectory(i).tobytes(), state=bytes(fl.tp_state(i, 1)[0]),
                path=_grids(fl, i)[0].tobytes(), goal=_grids(fl, i)[1].tobytes())


def _assert_same(a, b, what):
    for k in a:
        assert a[k] == b[k], (what, k)


def _twin(nav, n, nx, ny, robots, variant=None):
    """fleet A through the listed calls, fleet B through the range calls run by run, two consecutive cycles; asserts everything"""
    v = dict(VARIANTS[variant]) if variant else {}
    maps, old, cycles = _scene(n, nx, ny)
    maps = list(maps)
    robots = list(robots)
    others = [i for i in range(n) if i not in robots]
    if "boxed" in v:  # lethal cells 2 to 5 cells round the robot's cell: its outline (0.15 - 0.21 m from the centre) lies on them wherever it turns
        i = v["boxed"]
        m = maps[i].copy()
        cx, cy = int(cycles[0][i][0][0] / RES), int(cycles[0][i][0][1] / RES)
        m[cy - 5:cy + 6, cx - 5:cx + 6] = LETHAL
        m[cy - 1:cy + 2, cx - 1:cx + 2] = 0
        maps[i] = m
    wide = v.get("wide", (5,))
    A, B = (_fleet(nav, nx, ny, maps, wide, v.get("cfg", {})) for _ in range(2))
    try:
        for fl in (A, B):  # grids from an older plan on every robot: a call that leaves a robot alone leaves these
            fl.tp_update_plans(old, compute_dists=True)
        before = {i: _state(A, i) for i in others}
        for cyc in (0, 1):
            pos, vel = np.stack([cycles[cyc][i][0] for i in robots]), np.stack([cycles[cyc][i][1] for i in robots])
            plans = [np.zeros((0, 2)) if v.get("empty") == i else cycles[cyc][i][2] for i in robots]
            dists = cyc == 1  # the second cycle also runs updatePlan's own wavefronts (no within_robot bits) through the list
            A.tp_update_plans_list(robots, plans, compute_dists=dists)
            for first, count in _runs(robots):
                k = robots.index(first)
                B.tp_update_plans(plans[k:k + count], compute_dists=dists, first=first)
            if dists:
                for i in robots:
                    for ga, gb in zip(_grids(A, i), _grids(B, i)):
                        assert np.array_equal(ga, gb), (variant, nx, i, "updatePlan's grids")
            got = A.tp_find_best_path_list(robots, pos, vel)
            want = []
            for first, count in _runs(robots):
                k = robots.index(first)
                want += B.tp_find_best_path(pos[k:k + count], vel[k:k + count], first=first)
            assert len(got) == len(robots)
            for k, i in enumerate(robots):
                assert bytes(got[k]) == bytes(want[k]), (variant, nx, cyc, i, "result")
                _assert_same(_state(A, i), _state(B, i), (variant, nx, cyc, "robot", i))
            print(f"{variant} {nx}x{ny} cycle {cyc}: costs {[round(r.cost, 4) for r in got]} calls {[r.n_samples for r in got]}")
            if "boxed" in v and v["boxed"] in robots:
                assert A.tp_state(v["boxed"], 1)[0].flags & TP_ESCAPING, "the boxed-in robot did not enter escape mode"
        assert any(r.cost >= 0 and r.n_points > 0 for r in got), "no listed robot found a trajectory: the scene tells nothing"
        for i in others:  # nobody outside the list was touched
            _assert_same(before[i], _state(A, i), (variant, nx, "unlisted robot", i))
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ 1. parity of the two calls
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_listed_calls_equal_range_calls(nav, variant):
    _twin(nav, N_ROBOTS, 64, 64, LIST, variant)


# ------------------------------------------------------------------------------------------------ 2. every wavefront kernel, two grids + within
# words per row = ceil(width / 32) at 96 rows: k_bfs_rows<7> up to 7 words, k_bfs_rows2 from 21 to 32, k_bfs_global beyond
WAVEFRONT_WIDTHS = {120: "k_bfs_rows<7>", 648: "k_bfs_rows2", 1032: "k_bfs_global"}


def test_widths_take_the_kernels_named():
    words = {w: (w + 31) // 32 for w in WAVEFRONT_WIDTHS}
    assert words[120] <= 7 and 20 < words[648] <= 32 < words[1032]


@pytest.mark.parametrize("width", list(WAVEFRONT_WIDTHS))
def test_listed_calls_equal_range_calls_wavefronts(nav, width):
    _twin(nav, 3, width, 96, (1, 2))


# ------------------------------------------------------------------------------------------------ 3. edge lists and errors
@pytest.mark.parametrize("robots", [tuple(range(N_ROBOTS)), (5,), (N_ROBOTS - 1,)])
def test_full_list_and_single_robot(nav, robots):
    _twin(nav, N_ROBOTS, 64, 64, robots)


def test_empty_list_and_errors(nav):
    from navigation_amd import _lib as N
    import ctypes as C
    maps, old, cycles = _scene(N_ROBOTS, 64, 64)
    A = _fleet(nav, 64, 64, maps, cfg={})
    fresh = _fleet(nav, 64, 64, maps)  # never configured
    try:
        L = A.L
        u32 = lambda v: np.asarray(v, np.uint32)  # noqa: E731
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        A.tp_update_plans(old, compute_dists=True)
        pos, vel = np.stack([c[0] for c in cycles[0]]), np.stack([c[1] for c in cycles[0]])
        A.tp_find_best_path(pos, vel)  # every robot owns a cycle's state
        before = [_state(A, i) for i in range(N_ROBOTS)]

        def unchanged(what):
            for i in range(N_ROBOTS):
                _assert_same(before[i], _state(A, i), (what, i))

        # an empty list: no work, no error
        A.tp_update_plans_list([], [], compute_dists=True)
        assert A.tp_find_best_path_list([], np.zeros((0, 3)), np.zeros((0, 3))) == []
        unchanged("empty list")
        # malformed lists
        st, out = (N.RobotState * 2)(), (N.TpResult * 2)()
        xy, off = np.zeros((4, 2)), u32([0, 2, 4])
        for bad in ([2, 2], [3, 1], [1, N_ROBOTS]):
            assert L.navgpu_tp_update_plans_list(A.h, 2, p(u32(bad)), p(xy), p(off), 1) == NAVGPU_ERR_INVALID, bad
            assert L.navgpu_tp_find_best_path_list(A.h, 2, p(u32(bad)), st, out) == NAVGPU_ERR_INVALID, bad
        assert L.navgpu_tp_update_plans_list(A.h, 2, None, p(xy), p(off), 1) == NAVGPU_ERR_INVALID
        assert L.navgpu_tp_update_plans_list(A.h, 2, p(u32([1, 4])), p(xy), None, 1) == NAVGPU_ERR_INVALID
        assert L.navgpu_tp_update_plans_list(A.h, 2, p(u32([1, 4])), p(xy), p(u32([0, 3, 2])), 1) == NAVGPU_ERR_INVALID
        assert L.navgpu_tp_update_plans_list(A.h, N_ROBOTS + 1, p(u32(range(N_ROBOTS + 1))), p(xy), p(off), 1) == NAVGPU_ERR_INVALID
        assert L.navgpu_tp_find_best_path_list(A.h, 2, p(u32([1, 4])), None, out) == NAVGPU_ERR_INVALID
        assert L.navgpu_tp_find_best_path_list(A.h, 2, p(u32([1, 4])), st, None) == NAVGPU_ERR_INVALID
        unchanged("malformed lists")
        # a plan longer than max_plan on the second listed robot: nothing changed for the first either
        with pytest.raises(N.NavgpuError, match=r"\(-4\)"):
            A.tp_update_plans_list([1, 4], [cycles[1][1][2], np.zeros((MAX_PLAN + 1, 2))], compute_dists=True)
        unchanged("capacity")
        # before navgpu_tp_configure
        assert L.navgpu_tp_update_plans_list(fresh.h, 2, p(u32([1, 4])), p(xy), p(off), 0) == NAVGPU_ERR_STATE
        assert L.navgpu_tp_find_best_path_list(fresh.h, 2, p(u32([1, 4])), st, out) == NAVGPU_ERR_STATE
        # simple_attractor with an empty plan on the second listed robot
        A.configure_trajectory_planner(N.TpConfig(**dict(CFG, simple_attractor=1)))
        A.tp_update_plans_list([4], [np.zeros((0, 2))])
        before = [_state(A, i) for i in range(N_ROBOTS)]
        with pytest.raises(N.NavgpuError, match=r"\(-5\)"):
            A.tp_find_best_path_list([1, 4], pos[[1, 4]], vel[[1, 4]])
        unchanged("simple_attractor")
    finally:
        A.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------ 4. the control cycle
def _counted_cycle(fl, twin, ref, cfg, poses, vels, have, window, what):
    """test_gpu_tp_ros._cycle with the call's brackets counted: the downloads and reads round the call launch nothing that is bracketed"""
    fl.profile_reset()
    got, dec, grids = _cycle(fl, twin, ref, cfg, poses, vels, have, window, what)
    prof = fl.profile_read()
    step4 = [d.kind in (R.ROLLOUT, R.REACHED) for d in dec]
    probes = any(d.kind == R.REACHED for d in dec)
    print(f"{what}: k_bfs {prof['k_bfs'][1]} k_score {prof['k_score'][1]} step-4 robots {[i for i, s in enumerate(step4) if s]} probes {probes}")
    # ONE updatePlan / findBestPath for the call's robots, however they lie; k_tp_probe (one call for all candidates) is bracketed under k_score too
    assert prof["k_bfs"][1] == (1 if any(step4) else 0), (what, prof["k_bfs"])
    assert prof["k_score"][1] == (1 if any(step4) else 0) + (1 if probes else 0), (what, prof["k_score"])
    return got, dec, grids


def test_control_cycle_of_eight_is_one_launch_set(nav):
    """ROLLOUT, STOP, ROTATE, AT_GOAL, a blocked ROTATE and three NONE: robots 0, 1, 2 and 4 need step 4 and lie in two runs"""
    from navigation_amd import _lib as N
    window = _window(nav.lib())
    maps = [np.zeros((64, 64), np.uint8) for _ in range(8)]
    maps[4][:, 28] = LETHAL  # a corridor 0.35 m wide round x = 1.625: the wide robot stands across it and cannot turn
    maps[4][:, 36] = LETHAL
    fl, twin = _ros_fleet(nav, 8, maps, wide=(4,)), _ros_fleet(nav, 8, maps, wide=(4,))
    try:
        cfg = N.TpConfig(**CFG)
        fl.configure_tp_ros(**PARAMS)
        long_plan = _plan((0.3, 0.3), (2.7, 2.7), 0.0, yaw_step=0.01)
        short = _plan((0.5, 2.0), (1.5, 2.0), 0.0)
        plans = [_plan((0.5, 1.6), (2.9, 1.6), 0.0), long_plan, short, short, _plan((1.625, 0.8), (1.625, 1.6), 0.9), short, np.zeros((0, 3)),
                 _plan((2.6, 2.6), (3.0, 3.0), 0.0)]
        fl.tp_ros_set_plans(plans)
        ref = [R.Robot() for _ in range(8)]
        for r, pl in zip(ref, plans):
            r.set_plan(pl)
        old = [_plan((0.4, 0.4), (1.0, 0.4), 0.0)[:, :2]] * 8
        fl.tp_update_plans(old, compute_dists=True)
        for i in range(8):
            twin.tp_update_plan(i, old[i], compute_dists=True)
        end = long_plan[-1]
        poses = np.array([(0.5, 1.6, 0.0), (end[0] - 0.02, end[1] - 0.02, 0.8), (1.47, 2.0, 0.9), (1.47, 2.0, 0.02), (1.625, 1.58, 0.0), (1.0, 2.0, 0.0),
                          (1.0, 1.0, 0.0), (0.3, 0.3, 0.0)])
        vels = np.array([(0.2, 0.0, 0.0), (0.3, 0.0, 0.2)] + [(0.0, 0.0, 0.0)] * 6)
        have = [True, True, True, True, True, False, True, True]
        fl.profile(True)
        got, dec, _ = _counted_cycle(fl, twin, ref, cfg, poses, vels, have, window, "cycle 1")
        assert [g.branch for g in got] == [N.BRANCH_ROLLOUT, N.BRANCH_STOP, N.BRANCH_ROTATE, N.BRANCH_AT_GOAL, N.BRANCH_ROTATE, N.BRANCH_NONE,
                                           N.BRANCH_NONE, N.BRANCH_NONE]
        assert [g.ok for g in got] == [1, 1, 1, 1, 0, 0, 0, 0], [g.ok for g in got]
        assert [d.kind in (R.ROLLOUT, R.REACHED) for d in dec] == [True, True, True, False, True, False, False, False]
        poses[0] = (1.8, 1.6, 0.0)  # cycle 2: the persistent state carries through the listed calls
        poses[1] = (0.5, 0.5, 1.0)
        poses[2] = (1.2, 2.05, 0.9)
        got, dec, _ = _counted_cycle(fl, twin, ref, cfg, poses, vels, have, window, "cycle 2")
        assert got[0].branch == N.BRANCH_ROLLOUT and got[1].branch == N.BRANCH_STOP and got[2].branch == N.BRANCH_ROTATE
    finally:
        fl.close()
        twin.close()


def test_control_cycle_every_third_robot_at_its_goal(nav):
    from navigation_amd import _lib as N
    window = _window(nav.lib())
    n = 12
    maps = [np.zeros((64, 64), np.uint8) for _ in range(n)]
    fl, twin = _ros_fleet(nav, n, maps), _ros_fleet(nav, n, maps)
    try:
        cfg = N.TpConfig(**CFG)
        fl.configure_tp_ros(**PARAMS)
        short = _plan((0.5, 2.0), (1.5, 2.0), 0.0)
        plans = [short if i % 3 == 2 else _plan((0.5, 1.0 + 0.1 * i), (2.9, 1.0 + 0.1 * i), 0.0) for i in range(n)]
        fl.tp_ros_set_plans(plans)
        ref = [R.Robot() for _ in range(n)]
        for r, pl in zip(ref, plans):
            r.set_plan(pl)
        old = [_plan((0.4, 0.4), (1.0, 0.4), 0.0)[:, :2]] * n
        fl.tp_update_plans(old, compute_dists=True)
        for i in range(n):
            twin.tp_update_plan(i, old[i], compute_dists=True)
        poses = np.array([(1.47, 2.0, 0.02) if i % 3 == 2 else (0.5, 1.0 + 0.1 * i, 0.0) for i in range(n)])
        vels = np.array([(0.0, 0.0, 0.0) if i % 3 == 2 else (0.2, 0.0, 0.0) for i in range(n)])
        fl.profile(True)
        for cyc in (1, 2):
            got, dec, _ = _counted_cycle(fl, twin, ref, cfg, poses, vels, [True] * n, window, f"cycle {cyc}")
            assert [g.branch for g in got] == [N.BRANCH_ROLLOUT, N.BRANCH_ROLLOUT, N.BRANCH_AT_GOAL] * 4
            assert all(g.ok for g in got)
            for i in range(n):  # the robots move as commanded
                c, th = got[i].cmd_vel, poses[i, 2]
                poses[i] += np.array([c[0] * np.cos(th) - c[1] * np.sin(th), c[0] * np.sin(th) + c[1] * np.cos(th), c[2]]) * cfg.sim_period
                vels[i] = tuple(c)
    finally:
        fl.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 5. checkTrajectory(update_map)
def test_check_trajectories_update_map_is_one_listed_update(nav):
    from navigation_amd import _lib as N
    maps = [np.zeros((64, 64), np.uint8) for _ in range(6)]
    maps[5][:, 40] = LETHAL
    fl, twin = _ros_fleet(nav, 6, maps), _ros_fleet(nav, 6, maps)
    try:
        fl.configure_tp_ros(**PARAMS)
        plan = _plan((0.5, 1.6), (1.9, 1.6), 0.0)[:, :2]
        fl.tp_update_plans([plan] * 6, compute_dists=True)
        for i in range(6):
            twin.tp_update_plan(i, plan, compute_dists=True)
        inst = [0, 2, 5]
        poses = np.array([(0.62, 1.62, 0.1), (0.7, 1.5, 0.0), (1.2, 1.62, 0.0)])
        vels = np.array([(0.2, 0.0, 0.1), (0.0, 0.0, 0.0), (0.5, 0.0, 0.0)])
        samples = [np.array([(0.3, 0.0, 0.2), (0.0, 0.0, -0.8)]), np.array([(0.1, 0.0, 0.0)]), np.array([(0.55, 0.0, 0.0), (0.0, 0.0, 0.5), (-0.1, 0.0, 0.0)])]
        fl.profile(True)
        fl.profile_reset()
        costs, ok = fl.tp_ros_check_trajectories(inst, poses, vels, samples, update_map=True)
        prof = fl.profile_read()
        assert prof["k_bfs"][1] == 1 and prof["k_score"][1] == 1, (prof["k_bfs"], prof["k_score"])  # three runs of one robot, one updatePlan
        want = []
        for i, pose, vel, run in zip(inst, poses, vels, samples):
            twin.tp_update_plan(i, pose[None, :2], compute_dists=True)
            want += [twin.tp_score_trajectory(i, pose, vel, s) for s in run]
        print(f"costs {costs.tolist()} twin {want}")
        assert costs.tolist() == want and ok.tolist() == [w >= 0 for w in want]
        assert costs[0] >= 0 and costs[3] < 0  # robot 5 drives into its wall
        for gid in (N.GRID_PATH, N.GRID_GOAL):
            assert np.array_equal(fl.download(gid), twin.download(gid)), gid
    finally:
        fl.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 6. completing bounded MapGrids
def test_partial_grids_are_completed_in_one_listed_launch(nav):
    """a DWA fleet of six, robots 1, 3 and 4 with plans long enough for a bounded search: a download of the whole range, and a
    checkTrajectory whose probes leave the boxes of robots 1 and 4, each complete their robots in ONE wavefront launch"""
    from navigation_amd import _lib as N
    from test_gpu_cycle_list import _fleet as dwa_fleet, _scene as dwa_scene
    masters, sets = dwa_scene(120, 120)
    masters, n = masters[:6], 6
    partial = (1, 3, 4)
    pos, vel = np.stack([sets[0][i][0] for i in range(n)]), np.stack([sets[0][i][1] for i in range(n)])
    plans = []
    for i in range(n):
        d = np.arange(0.0, 3.0 if i in partial else 1.0, 0.05)
        plans.append(np.stack([pos[i, 0] + d * np.cos(pos[i, 2]), pos[i, 1] + d * np.sin(pos[i, 2])], 1))
    A, B = dwa_fleet(nav, 120, 120, "sweep", masters), dwa_fleet(nav, 120, 120, "whole_grids", masters)
    grids = (N.GRID_PATH, N.GRID_GOAL, N.GRID_GOAL_FRONT)
    try:
        for fl in (A, B):
            fl.set_plan()
            fl.find_best_path(pos, vel, plans)
        whole = (0, 119, 0, 119)
        assert [tuple(b) != whole for b in A.wavefront_boxes()] == [i in partial for i in range(n)]
        want = [B.download(g) for g in grids]
        A.profile(True)
        A.profile_reset()
        got = A.download(N.GRID_PATH)
        assert A.profile_read()["k_bfs"][1] == 1  # robots 1 | 3, 4: two runs, one launch
        assert np.array_equal(got, want[0])
        for g, w in zip(grids, want):  # (all three grids were completed by that launch)
            assert np.array_equal(A.download(g), w), g
        assert A.profile_read()["k_bfs"][1] == 1
        # a new cycle leaves 1, 3 and 4 partial again; probes far beyond the boxes of 1 and 4
        A.find_best_path(pos, vel, plans)
        A.profile_reset()
        ok, costs = A.check_trajectories([1, 4], [np.array([(3.0, 0.0, 0.0)], np.float32)] * 2)
        assert A.profile_read()["k_bfs"][1] == 1 and len(ok) == 2
        okb, costsb = B.check_trajectories([1, 4], [np.array([(3.0, 0.0, 0.0)], np.float32)] * 2)
        assert ok.tolist() == okb.tolist() and costs.tolist() == costsb.tolist()
        A.profile_reset()
        for g, w in zip(grids, want):
            assert np.array_equal(A.download(g), w), g
        assert A.profile_read()["k_bfs"][1] == 1  # robot 3 was still partial
    finally:
        A.close()
        B.close()
