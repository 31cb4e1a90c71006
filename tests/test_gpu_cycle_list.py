"""The planner cycle for a robot list (navgpu_planner_stage_list / _stage_poses_list / _cycle_list / _results_list) and the control cycle
that uses it.  Need a real MI355X.

Nothing in the cycle reduces across robots, so the bar is bit equality throughout: a fleet driven through the listed calls against a twin
driven through the range calls, contiguous run by contiguous run; and, for the robots outside the list, the fleet against itself before
the listed calls.  The control cycle's outputs are held against oracle/local_planner_oracle.py as tests/test_gpu_check_trajectories.py
holds them, and its launches are counted: one scoring launch for robots 0 and 2 driving (two contiguous runs of one robot each)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwa_reference_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

NAVGPU_ERR_INVALID, NAVGPU_ERR_CAPACITY, NAVGPU_ERR_STATE = -1, -4, -5
N_ROBOTS, MAX_PLAN = 8, 128
# sim_time 1.2 s: the staged reach is ~1.0 m, so a robot further than ~2.0 m from the end of its plan gets bounded MapGrids
BASE_CFG = dict(D.DEFAULTS, vx_samples=6, vy_samples=3, vth_samples=8, sim_time=1.2, sim_granularity=0.1, use_dwa=1, discretize_by_time=1)
# the scoring launches, on 120 x 120 maps (k_bfs_rows<7>)
SCORING = {
    "sweep": dict(),                                                       # k_score_prep_tab + k_score_sweep
    "general": dict(cfg=dict(discretize_by_time=0)),                       # k_score_prep_gen + k_score_gen<CHUNK>
    "fp9_rollout": dict(cfg=dict(use_dwa=0), fp=D.FP9),                    # nine vertices, the goal-limited sample window
    "agg": dict(agg=(1, 0, 0, 0), yshift=(0.0, 0.0, 0.0, 0.1)),            # k_score_gen_agg
    "sum_scores": dict(cfg=dict(sum_scores=1)),
    "whole_grids": dict(bounded=False),                                    # bounded MapGrids off: whole grids compared
}
# the wavefront kernels by map width at 96 rows, words per row = ceil(width / 32): bfs_rows_words gives k_bfs_rows<7> up to 7 words,
# <13> up to 13, <20> up to 20; launch_bfs_rows2 takes up to 32 words; k_bfs_global beyond
WAVEFRONT_WIDTHS = {120: "k_bfs_rows<7>", 232: "k_bfs_rows<13>", 424: "k_bfs_rows<20>", 648: "k_bfs_rows2", 1032: "k_bfs_global"}


def test_widths_take_the_kernels_named():
    words = {w: (w + 31) // 32 for w in WAVEFRONT_WIDTHS}
    assert words[120] <= 7 < words[232] <= 13 < words[424] <= 20 < words[648] <= 32 < words[1032]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


_SCENES = {}


def _scene(nx, ny):
    """N_ROBOTS maps with lethal cells near the robot (some samples collide), and three sets of inputs per robot: for the whole-fleet cycle,
    for the first listed cycle (new pose, velocity and plan) and for the second (new pose and velocity).  Even robots have long plans
    (bounded MapGrids), odd robots short ones (whole grids).  Computed once per map size and left unchanged."""
    if (nx, ny) in _SCENES:
        return _SCENES[(nx, ny)]
    rs = np.random.RandomState(1000 + nx)
    masters, sets = [], [[], [], []]
    for i in range(N_ROBOTS):
        x, y, th = rs.uniform(0.9, 1.6), rs.uniform(1.6, ny * D.RES - 1.6), rs.uniform(-0.25, 0.25)
        cells = np.zeros((ny, nx), np.uint8)
        for j in range(6):
            a, d = rs.uniform(0, 2 * np.pi), rs.uniform(0.4, 0.9) / D.RES
            cells[int(y / D.RES + d * np.sin(a)), int(x / D.RES + d * np.cos(a))] = D.LETHAL
        m = D.inflate(cells)
        m.setflags(write=False)
        masters.append(m)
        for s in range(3):
            pos = np.array([x + 0.04 * s, y + 0.015 * s, th + 0.05 * s], np.float32)
            vel = np.array([rs.uniform(0.1, 0.4), 0.0, rs.uniform(-0.3, 0.3)], np.float32)
            if s < 2:  # the second listed cycle keeps the plan of the first
                length = rs.uniform(2.6, 3.3) if i % 2 == 0 else rs.uniform(0.8, 1.5)
                d = np.arange(0.0, length, 0.05)
                heading = th + rs.uniform(-0.15, 0.15)
                plan = np.stack([pos[0] + d * np.cos(heading), pos[1] + d * np.sin(heading)], 1)
            sets[s].append((pos, vel, plan))
    _SCENES[(nx, ny)] = (masters, sets)
    return _SCENES[(nx, ny)]


def _fleet(nav, nx, ny, variant, masters):
    from navigation_amd import _lib as N
    v = SCORING[variant]
    fl = nav.Fleet(len(masters), nx, ny, D.RES, layers=N.LAYER_OBSTACLE, keep_sample_costs=True, max_sim_steps=32, max_plan=MAX_PLAN)
    fl.configure_planner(nav.DwaConfig(**dict(BASE_CFG, **v.get("cfg", {}))))
    fl.set_footprint(v.get("fp", D.FP4))
    fl.upload(N.GRID_MASTER, np.stack(masters))
    for m, a, y in zip(D.MAP_GRID_CRITICS, v.get("agg", (0, 0, 0, 0)), v.get("yshift", (0, 0, 0, 0))):
        if a or y:
            fl.set_map_grid_options(m, D.AGGREGATIONS[a], y)
    fl.set_bounded_map_grids(1 if v.get("bounded", True) else 0)
    return fl


def _runs(robots):
    """the contiguous runs (first, count) of a strictly increasing list"""
    runs = []
    for r in robots:
        if runs and runs[-1][0] + runs[-1][1] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    return [tuple(r) for r in runs]


def _state(fl, i):
    """what a cycle leaves for robot i, as bytes - without the MapGrids, whose download completes a bounded search"""
    flags, prev = fl.oscillation(i, 1)
    return dict(result=bytes(fl.results(i, 1)[0]), trajectory=fl.trajectory(i).tobytes(), samples=b"".join(a.tobytes() for a in fl.samples(i)),
                oscillation=flags.tobytes() + prev.tobytes(), box=fl.wavefront_boxes(i, 1).tobytes(), levels=fl.wavefront_levels(i, 1).tobytes())


def _grids(fl, i):
    from navigation_amd import _lib as N
    return [fl.download(g, i, 1)[0] for g in (N.GRID_PATH, N.GRID_GOAL, N.GRID_GOAL_FRONT)]


def _assert_same(a, b, what):
    for k in a:
        assert a[k] == b[k], (what, k)


def _twin_cycles(nav, nx, ny, variant, robots):
    """fleet A through the listed calls, fleet B through the range calls run by run; returns nothing, asserts everything"""
    masters, sets = _scene(nx, ny)
    robots = list(robots)
    others = [i for i in range(N_ROBOTS) if i not in robots]
    A, B = _fleet(nav, nx, ny, variant, masters), _fleet(nav, nx, ny, variant, masters)
    try:
        for fl in (A, B):  # a whole-fleet range cycle first: every robot owns state
            fl.set_plan()
            fl.find_best_path(np.stack([s[0] for s in sets[0]]), np.stack([s[1] for s in sets[0]]), [s[2] for s in sets[0]])
        grids_before = {i: _grids(A, i) for i in others}  # (the download completes a bounded search: before the rest is looked at)
        before = {i: _state(A, i) for i in others}
        for i in others:
            _grids(B, i)  # (the twin completes the same robots' grids)
        for cyc in (1, 2):
            pos, vel = np.stack([sets[cyc][i][0] for i in robots]), np.stack([sets[cyc][i][1] for i in robots])
            if cyc == 1:
                A.stage_planner_list(robots, pos, vel, [sets[1][i][2] for i in robots])
            else:  # plans unchanged: poses only
                A.stage_poses_list(robots, pos, vel)
            A.planner_cycle_list(robots)
            got = A.results_list(robots)
            for first, count in _runs(robots):
                k = robots.index(first)
                if cyc == 1:
                    B.stage_planner(pos[k:k + count], vel[k:k + count], [sets[1][i][2] for i in robots[k:k + count]], first=first)
                else:
                    B.stage_poses(pos[k:k + count], vel[k:k + count], first=first)
            for first, count in _runs(robots):
                B.planner_cycle(first, count)
            for k, i in enumerate(robots):
                sa, sb = _state(A, i), _state(B, i)
                _assert_same(sa, sb, (variant, nx, cyc, "robot", i))
                assert bytes(got[k]) == sb["result"], (variant, nx, cyc, i, "results_list")
        valid = [r.cost >= 0 for r in got]
        assert any(valid), "no listed robot found a trajectory: the scene tells nothing"
        boxes = A.wavefront_boxes()
        for i in robots:  # the three MapGrids: inside the robot's box (a bounded search is exact there), whole where the search was whole
            x0, x1, y0, y1 = A.wavefront_boxes(i, 1)[0]
            if not SCORING[variant].get("bounded", True):
                assert (x0, x1, y0, y1) == (0, nx - 1, 0, ny - 1)
            for ga, gb in zip(_grids(A, i), _grids(B, i)):
                assert np.array_equal(ga[y0:y1 + 1, x0:x1 + 1], gb[y0:y1 + 1, x0:x1 + 1]), (variant, nx, i, "MapGrid")
        for i in others:  # nobody outside the list was touched
            _assert_same(before[i], _state(A, i), (variant, nx, "unlisted robot", i))
            for g0, g1 in zip(grids_before[i], _grids(A, i)):
                assert np.array_equal(g0, g1), (variant, nx, "unlisted robot's MapGrid", i)
        if any(i % 2 == 0 for i in robots) and SCORING[variant].get("bounded", True) and not SCORING[variant].get("agg"):
            assert any(tuple(b) != (0, nx - 1, 0, ny - 1) for b in boxes[robots]), "no listed robot ran a bounded search"
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ a. twin fleets
@pytest.mark.parametrize("variant", list(SCORING))
def test_listed_cycle_equals_range_cycles_scoring(nav, variant):
    _twin_cycles(nav, 120, 120, variant, (0, 2, 3, 7))


@pytest.mark.parametrize("width", [w for w in WAVEFRONT_WIDTHS if w != 120])
def test_listed_cycle_equals_range_cycles_wavefronts(nav, width):
    _twin_cycles(nav, width, 96, "sweep", (0, 2, 3, 7))


# ------------------------------------------------------------------------------------------------ b. full list, single robots
@pytest.mark.parametrize("robots", [tuple(range(N_ROBOTS)), (5,), (N_ROBOTS - 1,)])
def test_full_list_and_single_robot(nav, robots):
    _twin_cycles(nav, 120, 120, "sweep", robots)


def test_result_slots_across_the_in_flight_switch(nav):
    """Two whole-fleet cycles with two cycles in flight, back to one, then a listed cycle: the listed cycle shares the range cycle's code
    and must never flip the result slot.  Everything read is byte-equal to a twin that runs the listed step as range calls, and the
    robots outside the list keep the results of the second whole-fleet cycle."""
    from navigation_amd import _lib as N
    masters, sets = _scene(120, 120)
    robots = [0, 2, 3, 7]
    A, B = _fleet(nav, 120, 120, "sweep", masters), _fleet(nav, 120, 120, "sweep", masters)
    try:
        read = {}
        for fl in (A, B):
            fl.set_plan()
            fl.set_cycles_in_flight(2)
            for s in (0, 1):
                fl.stage_planner(np.stack([x[0] for x in sets[s]]), np.stack([x[1] for x in sets[s]]), [x[2] for x in sets[s]])
                fl.planner_cycle()
            previous = list(fl.results_previous_into((N.PlanResult * N_ROBOTS)()))
            latest = fl.results()
            fl.set_cycles_in_flight(1)
            pos, vel = np.stack([sets[2][i][0] for i in robots]), np.stack([sets[2][i][1] for i in robots])
            plans = [sets[2][i][2] for i in robots]
            if fl is A:
                fl.stage_planner_list(robots, pos, vel, plans)
                fl.planner_cycle_list(robots)
                listed = fl.results_list(robots)
            else:
                listed = []
                for first, count in _runs(robots):
                    k = robots.index(first)
                    fl.stage_planner(pos[k:k + count], vel[k:k + count], plans[k:k + count], first=first)
                    fl.planner_cycle(first, count)
                    listed += fl.results(first, count)
            read["A" if fl is A else "B"] = {k: [bytes(r) for r in v] for k, v in dict(previous=previous, latest=latest, listed=listed, after=fl.results()).items()}
        _assert_same(read["A"], read["B"], "twins")
        a = read["A"]
        assert a["previous"] != a["latest"], "both whole-fleet cycles gave the same results: the slots cannot be told apart"
        for i in range(N_ROBOTS):
            assert a["after"][i] == (a["listed"][robots.index(i)] if i in robots else a["latest"][i]), i
    finally:
        A.close()
        B.close()


def test_pose_stage_across_a_chunk_boundary(nav):
    """70 robots, more than the 64 a pose chunk holds: stage_poses_list of every robot but 1 and 66 takes two chunks and its runs cross
    entry 64; the twin's run [2, 66) crosses the range form's chunk boundary as well."""
    masters, sets = _scene(120, 120)
    n = 70
    robots = [i for i in range(n) if i not in (1, 66)]
    of = lambda s, i: sets[s][i % N_ROBOTS]  # noqa: E731  (the scene's eight robots, over again)
    many = [masters[i % N_ROBOTS] for i in range(n)]
    A, B = _fleet(nav, 120, 120, "sweep", many), _fleet(nav, 120, 120, "sweep", many)
    try:
        for fl in (A, B):
            fl.set_plan()
            fl.find_best_path(np.stack([of(0, i)[0] for i in range(n)]), np.stack([of(0, i)[1] for i in range(n)]), [of(0, i)[2] for i in range(n)])
        before = {i: _state(A, i) for i in (1, 66)}
        pos, vel = np.stack([of(1, i)[0] for i in robots]), np.stack([of(1, i)[1] for i in robots])
        A.stage_poses_list(robots, pos, vel)
        A.planner_cycle_list(robots)
        assert _runs(robots) == [(0, 1), (2, 64), (67, 3)]
        for first, count in _runs(robots):
            k = robots.index(first)
            B.stage_poses(pos[k:k + count], vel[k:k + count], first=first)
            B.planner_cycle(first, count)
        for i in robots:
            _assert_same(_state(A, i), _state(B, i), ("robot", i))
        for i in (1, 66):
            _assert_same(before[i], _state(A, i), ("unlisted robot", i))
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ c. errors
def test_errors(nav):
    from navigation_amd import _lib as N
    masters, sets = _scene(120, 120)
    A, B = _fleet(nav, 120, 120, "sweep", masters), _fleet(nav, 120, 120, "sweep", masters)
    try:
        L = A.L
        u32 = lambda v: np.asarray(v, np.uint32)  # noqa: E731
        pos, vel = np.stack([s[0] for s in sets[0]]), np.stack([s[1] for s in sets[0]])
        res = (N.PlanResult * N_ROBOTS)()

        def cycle(inst):
            inst = u32(inst)
            return L.navgpu_planner_cycle_list(A.h, len(inst), inst.ctypes.data)

        assert cycle([0, 2]) == NAVGPU_ERR_STATE  # configured, nothing staged
        inst = u32([0, 2])
        assert L.navgpu_planner_stage_poses_list(A.h, 2, inst.ctypes.data, pos.ctypes.data, vel.ctypes.data) == NAVGPU_ERR_STATE
        # a plan for robots 0 .. 6 only: stage_poses_list names the robot that has none
        for fl in (A, B):
            fl.set_plan()
            fl.stage_planner(pos[:7], vel[:7], [s[2] for s in sets[0][:7]])
        inst = u32([1, 7])
        assert L.navgpu_planner_stage_poses_list(A.h, 2, inst.ctypes.data, pos.ctypes.data, vel.ctypes.data) == NAVGPU_ERR_STATE
        assert b"instance 7" in L.navgpu_last_error()
        for fl in (A, B):
            fl.stage_planner(pos, vel, [s[2] for s in sets[0]])
        # malformed lists, every call
        packed = np.ascontiguousarray(np.concatenate([s[2] for s in sets[1]]))
        states = (N.RobotState * N_ROBOTS)()
        off = 0
        for k in range(N_ROBOTS):
            states[k].pos[:] = sets[1][k][0].tolist()
            states[k].vel[:] = sets[1][k][1].tolist()
            states[k].plan_first, states[k].plan_count = off, len(sets[1][k][2])
            off += len(sets[1][k][2])
        sp = C.cast(states, C.c_void_p)

        def calls(n, ptr):
            return (L.navgpu_planner_stage_list(A.h, n, ptr, sp, packed.ctypes.data, len(packed)),
                    L.navgpu_planner_stage_poses_list(A.h, n, ptr, pos.ctypes.data, vel.ctypes.data),
                    L.navgpu_planner_cycle_list(A.h, n, ptr),
                    L.navgpu_planner_results_list(A.h, n, ptr, C.cast(res, C.c_void_p)))

        for bad in ([1, 1], [2, 1], [1, N_ROBOTS], list(range(N_ROBOTS)) + [N_ROBOTS]):
            arr = u32(bad)
            assert calls(len(arr), arr.ctypes.data) == (NAVGPU_ERR_INVALID,) * 4, bad
        arr = u32([0, 1])
        assert calls(0, arr.ctypes.data) == (NAVGPU_ERR_INVALID,) * 4
        assert calls(2, None) == (NAVGPU_ERR_INVALID,) * 4
        assert L.navgpu_planner_stage_list(A.h, 2, arr.ctypes.data, None, packed.ctypes.data, len(packed)) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_stage_list(A.h, 2, arr.ctypes.data, sp, None, len(packed)) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_stage_poses_list(A.h, 2, arr.ctypes.data, None, vel.ctypes.data) == NAVGPU_ERR_INVALID
        assert L.navgpu_planner_results_list(A.h, 2, arr.ctypes.data, None) == NAVGPU_ERR_INVALID
        # stage_list is all or nothing: one robot's plan_count 0 / above max_plan gives the range form's code, and nothing is staged
        arr = u32([0, 2, 3])
        for count, code in ((0, NAVGPU_ERR_INVALID), (MAX_PLAN + 1, NAVGPU_ERR_CAPACITY)):
            keep = states[1].plan_count
            states[1].plan_count = count
            assert L.navgpu_planner_stage_list(A.h, 3, arr.ctypes.data, sp, packed.ctypes.data, len(packed)) == code
            assert L.navgpu_planner_stage(B.h, 0, 3, sp, packed.ctypes.data, len(packed)) == code
            states[1].plan_count = keep
        states[2].plan_first = len(packed)  # beyond the packed plans
        assert L.navgpu_planner_stage_list(A.h, 3, arr.ctypes.data, sp, packed.ctypes.data, len(packed)) == NAVGPU_ERR_INVALID
        A.planner_cycle_list([0, 2, 3])  # A made the failing calls, its twin made none of the listed ones
        B.planner_cycle(0, 1)
        B.planner_cycle(2, 2)
        assert [bytes(r) for r in A.results_list([0, 2, 3])] == [bytes(r) for r in B.results(0, 1) + B.results(2, 2)]
        # two cycles in flight take whole-fleet range cycles only
        A.set_cycles_in_flight(2)
        assert cycle([0, 2]) == NAVGPU_ERR_STATE and cycle(list(range(N_ROBOTS))) == NAVGPU_ERR_STATE
        A.set_cycles_in_flight(1)
        assert cycle([0, 2]) == 0
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ d. the control cycle
def _control_scenario(nav, want_branch, collides=()):
    """tests/test_gpu_check_trajectories.py's scenario for any list of branches: robots on 120 x 120 maps - configuration, limits, maps, stored
    plans, and the poses / velocities of a warm-up cycle (every robot half a metre short of where it will stand, driving: DWA for all,
    which computes the MapGrids checkTrajectory reads) and of the cycle that follows it.  collides: robots whose rotation is in collision."""
    from navigation_amd import _lib as N, synth
    n, res = 120, synth.RES
    cfg = nav.DwaConfig(vx_samples=8, vy_samples=3, vth_samples=9, sim_time=1.2, sim_granularity=0.1, discretize_by_time=1)
    lim = dict(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, rot_stopped_vel=0.01, trans_stopped_vel=0.01, max_rot_vel=cfg.max_rot_vel,
               min_rot_vel=cfg.min_rot_vel, acc_lim_x=cfg.acc_lim_x, acc_lim_y=cfg.acc_lim_y, acc_lim_theta=cfg.acc_lim_theta,
               sim_period=cfg.sim_period, prune_plan=1, latch_xy_goal_tolerance=0)
    goal = np.array([3.0, 3.0, 0.5])
    masters = []
    for k in range(len(want_branch)):
        cells = np.zeros((n, n), np.uint8)
        cells[10:110, 100] = D.LETHAL
        if k in collides:  # a closed band of lethal cells through the footprint's outline: the rotation collides at its first point
            yy, xx = np.mgrid[0:n, 0:n]
            d = np.hypot((xx + 0.5) * res - (goal[0] + 0.03), (yy + 0.5) * res - goal[1])
            cells[(d >= 0.21) & (d <= 0.31)] = D.LETHAL
        masters.append(D.inflate(cells))
    s = np.linspace(0.0, 1.6, 33)
    plans, pose, vel = [], np.zeros((len(want_branch), 3)), np.zeros((len(want_branch), 3))
    warm_pose, warm_vel = np.zeros_like(pose), np.zeros_like(vel)
    for k, b in enumerate(want_branch):
        if b == N.BRANCH_DWA:  # a plan leading away from the robot
            ang = 0.4 * (k % 6)
            plans.append(np.stack([goal[0] + s * np.cos(ang), goal[1] + s * np.sin(ang), np.full_like(s, ang)], 1))
            pose[k] = (goal[0], goal[1], ang + 0.1)
            vel[k] = (0.2, 0.0, 0.0)
            warm_pose[k] = (goal[0] - 0.5 * np.cos(ang), goal[1] - 0.5 * np.sin(ang), ang)
        else:  # a plan that ends at `goal`, the robot 3 cm from it
            plans.append(np.stack([goal[0] - s[::-1] * np.cos(goal[2]), goal[1] - s[::-1] * np.sin(goal[2]), np.full_like(s, goal[2])], 1))
            pose[k] = (goal[0] + 0.03, goal[1], goal[2] + (0.0 if b == N.BRANCH_AT_GOAL else 0.9 if k in collides else -0.7))
            vel[k] = (0.3, 0.0, 0.2) if b == N.BRANCH_STOP else (0.0, 0.0, 0.0)
            warm_pose[k] = (goal[0] - 0.5 * np.cos(goal[2]), goal[1] - 0.5 * np.sin(goal[2]), goal[2])
        warm_vel[k] = (0.2, 0.0, 0.0)
    return dict(n=n, res=res, cfg=cfg, lim=lim, masters=masters, plans=plans, warm=(warm_pose, warm_vel), pose=pose, vel=vel)


def _run_control_cycles(nav, orc, want_branch, collides, resident, want_ok):
    """three control cycles against the oracle; the launches of the cycles behind the warm-up are counted"""
    from navigation_amd import _lib as N, synth
    from oracle import local_planner_oracle as lpo
    sc = _control_scenario(nav, want_branch, collides)
    n, res, cfg, lim, masters, plans = (sc[k] for k in ("n", "res", "cfg", "lim", "masters", "plans"))
    n_inst = len(want_branch)
    pose, vel = sc["pose"], sc["vel"]
    fl = nav.Fleet(n_inst, n, n, res, layers=N.LAYER_OBSTACLE, max_sim_steps=32, max_plan=256)
    try:
        fl.configure_planner(cfg)
        fl.set_footprint(synth.FOOTPRINT)
        fl.upload(N.GRID_MASTER, np.stack(masters))
        fl.configure_local_planner(**lim)
        if resident:
            fl.reserve_global_plans(64)
            fl.set_global_plans(plans)
        oracles = []
        for k in range(n_inst):
            o = lpo.DwaPlannerRos(orc.DwaPlanner(masters[k], res, 0.0, 0.0, orc.DwaConfig(**cfg.as_dict())), lim, n, n, res, synth.FOOTPRINT)
            o.set_plan(plans[k], None)
            oracles.append(o)
            if k not in resident:
                fl.set_global_plan(k, plans[k], None)  # (a resident robot is back on the host path)
        fl.profile(True)
        for cyc in range(3):  # the warm-up, then two consecutive cycles: rotating_to_goal and the latch carry over
            p, v = sc["warm"] if cyc == 0 else (pose, vel)
            fl.profile_reset()
            got = fl.compute_velocity_commands(p, v)
            prof = fl.profile_read()
            # ONE launch of each for the call's DWA robots, however they lie; one k_check_traj for its stop / rotate candidates
            n_check = sum(1 for b in want_branch if b in (N.BRANCH_STOP, N.BRANCH_ROTATE))
            assert prof["k_score"][1] == 1 and prof["k_select"][1] == 1, (cyc, prof["k_score"], prof["k_select"])
            assert prof["k_check_traj"][1] == (0 if cyc == 0 or not n_check else 1), cyc
            for k in range(n_inst):
                want = oracles[k].compute_velocity_commands(p[k], v[k])
                g = got[k]
                assert bool(g.ok) == bool(want["ok"]) and g.branch == want["branch"], (cyc, k, g.ok, g.branch, want)
                assert tuple(g.cmd_vel) == tuple(float(x) for x in want["cmd"]), (cyc, k, tuple(g.cmd_vel), want["cmd"])
                assert g.local_plan_points == want["local_plan_points"] and g.trajectory_points == want["trajectory_points"], (cyc, k)
            if cyc == 0:
                assert all(g.branch == N.BRANCH_DWA for g in got), [g.branch for g in got]
                continue
            if cyc == 1:
                assert [g.branch for g in got] == want_branch
                assert [bool(g.ok) for g in got] == want_ok
            for k in range(n_inst):  # the robots move as commanded
                c, th = got[k].cmd_vel, pose[k, 2]
                pose[k, 0] += (c[0] * np.cos(th) - c[1] * np.sin(th)) * cfg.sim_period
                pose[k, 1] += (c[0] * np.sin(th) + c[1] * np.cos(th)) * cfg.sim_period
                pose[k, 2] += c[2] * cfg.sim_period
                vel[k] = tuple(c)
    finally:
        fl.close()


@pytest.mark.parametrize("resident", [(), (0, 1, 2, 3, 4, 5), (1, 3, 4)], ids=["host_path", "resident", "mixed"])
def test_control_cycle_runs_its_dwa_robots_in_one_cycle(nav, orc, resident):
    """DWA / STOP / DWA / ROTATE in collision / AT_GOAL / ROTATE: robots 0 and 2 drive, two contiguous runs, one scoring launch.  With
    robots 1, 3 and 4 resident both staging sets are lists too."""
    from navigation_amd import _lib as N
    want_branch = [N.BRANCH_DWA, N.BRANCH_STOP, N.BRANCH_DWA, N.BRANCH_ROTATE, N.BRANCH_AT_GOAL, N.BRANCH_ROTATE]
    _run_control_cycles(nav, orc, want_branch, (3,), resident, [True, True, True, False, True, True])


def test_control_cycle_every_third_robot_at_its_goal(nav, orc):
    from navigation_amd import _lib as N
    want_branch = [N.BRANCH_DWA, N.BRANCH_DWA, N.BRANCH_AT_GOAL] * 4
    _run_control_cycles(nav, orc, want_branch, (), (), [True] * 12)


# ------------------------------------------------------------------------------------------------ e. trajectory cloud
def test_trajectory_cloud_follows_the_list(nav):
    """robots 2 (listed) and 5 (not) enabled: the listed robot's cloud is its twin's, the other's read call returns what it returned before"""
    masters, sets = _scene(120, 120)
    robots = [0, 2, 3, 7]
    A, B = _fleet(nav, 120, 120, "sweep", masters), _fleet(nav, 120, 120, "sweep", masters)
    try:
        for fl in (A, B):
            fl.set_trajectory_cloud(True, 2, 1)
            fl.set_trajectory_cloud(True, 5, 1)
            fl.set_plan()
            fl.find_best_path(np.stack([s[0] for s in sets[0]]), np.stack([s[1] for s in sets[0]]), [s[2] for s in sets[0]])
        cloud5, terms5 = A.trajectory_cloud(5), A.sample_terms(5)
        assert len(cloud5) > 0
        pos, vel = np.stack([sets[1][i][0] for i in robots]), np.stack([sets[1][i][1] for i in robots])
        A.stage_planner_list(robots, pos, vel, [sets[1][i][2] for i in robots])
        A.planner_cycle_list(robots)
        for first, count in _runs(robots):
            k = robots.index(first)
            B.stage_planner(pos[k:k + count], vel[k:k + count], [sets[1][i][2] for i in robots[k:k + count]], first=first)
            B.planner_cycle(first, count)
        a, b = A.trajectory_cloud(2), B.trajectory_cloud(2)
        assert len(a) > 0 and a.tobytes() == b.tobytes()
        assert A.sample_terms(2).tobytes() == B.sample_terms(2).tobytes()
        assert A.trajectory_cloud(5).tobytes() == cloud5.tobytes() and A.sample_terms(5).tobytes() == terms5.tobytes()
    finally:
        A.close()
        B.close()
