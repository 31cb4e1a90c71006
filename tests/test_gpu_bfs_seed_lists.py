"""Wavefront seed lists (navgpu_planner_set_seed_lists): a cycle's k_samples turns each robot's plan into the seed cells of its three
MapGrids and the wavefront items scatter them, instead of every item walking the plan.  Need a real MI355X.

Every case builds two fleets on the same scenes, lists on and lists off, and holds the three MapGrids of every robot bit for bit
against each other and against the oracle; navgpu_planner_wavefront_levels, the boxes and the planner results (the oracle keeps no
level count) bit for bit between the two fleets.  navgpu_planner_seed_list_counts says which wavefronts had a list, and with how
many cells: that is held against the seeding rule restated in numpy below.

One map size per kernel, the smallest that launch_bfs' dispatch routes to it (words per row = ceil(nx / 32): k_bfs_rows up to 20,
k_bfs_rows2 up to 32, k_bfs_global beyond), 48 rows each.  The scenes (one robot each) lie in the first 64 columns:

    point      one pose
    metre      two poses 1 m apart, interpolated poses between them (adjustPlanResolution): 17 path seeds
    window     starts off the map, then in NO_INFORMATION, becomes valid, runs into NO_INFORMATION again and goes on: [f, e)
    off_map    no pose on the map
    unknown    every pose in NO_INFORMATION
    dense      30 poses a cell apart: only the goal_front plan's last segment (its last pose moved 0.325 m on) gets interpolated
    long       two segments of 2.5 m and 2 m through a wall: 84 path seeds (the capacity case's robot that does not fit)
    near       the robot next to the end of its plan: whole grids also in the bounded mode
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu

LETHAL, NOINFO = 254, 255
NO_LIST = 0xFFFFFFFF
NY = 48
SIZES = {"k_bfs_rows": 64, "k_bfs_rows2": 648, "k_bfs_global": 1032}
SCENES = ("point", "metre", "window", "off_map", "unknown", "dense", "long", "near")


def test_sizes_take_the_kernels_named():
    words = {k: (nx + 31) // 32 for k, nx in SIZES.items()}
    assert words["k_bfs_rows"] <= 20 < words["k_bfs_rows2"] <= 32 < words["k_bfs_global"]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _cells(points, res):
    """poses at the centres of the given (fractional) cells"""
    return (np.asarray(points, np.float64).reshape(-1, 2) + 0.5) * res


def _master(nx):
    m = np.zeros((NY, nx), np.uint8)
    m[:, 0:4] = NOINFO
    m[26:35, 36:40] = NOINFO
    m[5:21, 50] = LETHAL
    m[40:47, 30] = LETHAL
    m.setflags(write=False)
    return m


def _scene_inputs(res):
    """plan and pose per scene, in SCENES' order; the second plan set gives every robot its neighbour's plan"""
    plans = {
        "point": _cells([[45, 12]], res),
        "metre": _cells([[20, 40], [40, 40]], res),
        "window": _cells([[x, 30] for x in np.arange(-6, 75, 5)], res),
        "off_map": _cells([[-10, -10], [-5, -3]], res),
        "unknown": _cells([[1, 10], [2, 20]], res),
        "dense": _cells(np.stack([np.linspace(8, 37, 30), np.linspace(6, 20, 30)], 1), res),
        "long": _cells([[10, 44], [60, 44], [60, 4]], res),
        "near": _cells([[20, 10], [30, 10]], res),
    }
    robots = {"point": (8, 12), "metre": (12, 38), "window": (10, 22), "off_map": (20, 20), "unknown": (30, 24), "dense": (6, 5), "long": (12, 30),
              "near": (28, 10)}
    pos = np.array([[(robots[s][0] + 0.5) * res, (robots[s][1] + 0.5) * res, 0.2] for s in SCENES], np.float32)
    first = [plans[s] for s in SCENES]
    return pos, [first, first[1:] + first[:1]]


_REF = {}


def _reference(nav, orc, nx, allow_unknown):
    """masters, poses, the two plan sets and, per plan set and robot, the oracle's three MapGrids: once per (size, allow_unknown)"""
    from navigation_amd import synth
    key = (nx, allow_unknown)
    if key not in _REF:
        res = synth.RES
        pos, plan_sets = _scene_inputs(res)
        cfg = _cfg(nav, allow_unknown)
        ocfg = orc.DwaConfig(**cfg.as_dict())
        master = _master(nx)
        grids = []
        for plans in plan_sets:
            per_robot = []
            for k, plan in enumerate(plans):
                p = orc.DwaPlanner(master, res, 0.0, 0.0, ocfg)
                p.set_plan()
                p.cycle(pos[k], np.zeros(3, np.float32), plan, synth.FOOTPRINT)
                per_robot.append([p.grid(w).reshape(NY, nx).copy() for w in range(3)])
            grids.append(per_robot)
        _REF[key] = (master, pos, plan_sets, grids)
    return _REF[key]


def _cfg(nav, allow_unknown):
    return nav.DwaConfig(vx_samples=3, vy_samples=1, vth_samples=3, sim_time=0.5, sim_granularity=0.1, discretize_by_time=1, allow_unknown=allow_unknown)


def _fleet(nav, nx, allow_unknown, lists, bounded=True, capacity=None):
    from navigation_amd import _lib as N, synth
    n = len(SCENES)
    fl = nav.Fleet(n, nx, NY, synth.RES, layers=N.LAYER_OBSTACLE, keep_sample_costs=True, max_sim_steps=16, max_plan=32)
    fl.configure_planner(_cfg(nav, allow_unknown))
    fl.set_footprint(synth.FOOTPRINT)
    fl.upload(N.GRID_MASTER, np.stack([_master(nx)] * n))
    fl.set_bounded_map_grids(bounded)
    fl.set_seed_lists(lists)
    if capacity is not None:
        fl.set_seed_list_capacity(capacity)
    fl.set_plan()
    return fl


def _expected_counts(orc, master, plan, res):
    """the seed cells of the path and goal wavefronts by the rule (map_grid.cpp:160-233): the adjusted plan's poses from the first
    valid one, f, up to the first invalid one after it, e (path); the pose e - 1 (goal)"""
    ny, nx = master.shape
    adj = orc.adjust_plan(plan, res)
    valid = []
    for x, y in adj:
        on = x >= 0.0 and y >= 0.0 and int(x / res) < nx and int(y / res) < ny
        valid.append(bool(on and master[int(y / res), int(x / res)] != NOINFO))
    if True not in valid:
        return 0, 0
    f = valid.index(True)
    e = valid.index(False, f) if False in valid[f:] else len(valid)
    return e - f, 1


def _compare(orc, on, off, ref_grids, robots, what, master, plans, capacity=1024):
    """the two fleets against each other and the oracle, for the given robots (after the cycle under test)"""
    from navigation_amd import _lib as N, synth
    lv_on, lv_off = on.wavefront_levels(), off.wavefront_levels()
    assert np.array_equal(lv_on[robots], lv_off[robots]), (what, "levels", lv_on.tolist(), lv_off.tolist())
    assert np.array_equal(on.wavefront_boxes()[robots], off.wavefront_boxes()[robots]), (what, "boxes")
    counts = on.seed_list_counts()
    for k in robots:
        n_path, n_goal = _expected_counts(orc, master, plans[k], synth.RES)
        want_path = n_path if n_path <= capacity else NO_LIST
        print(f"{what} {SCENES[k]}: levels {lv_on[k].tolist()} seed cells {counts[k].tolist()} expected path {n_path} goal {n_goal}")
        assert counts[k, 0] == want_path and counts[k, 1] == n_goal and counts[k, 2] in (0, 1), (what, SCENES[k], counts[k].tolist(), n_path, n_goal)
    assert (off.seed_list_counts() == NO_LIST).all(), (what, "the fleet without lists wrote some")
    for gid, which in ((N.GRID_PATH, 0), (N.GRID_GOAL, 1), (N.GRID_GOAL_FRONT, 2)):
        g_on, g_off = on.download(gid), off.download(gid)  # (completes the bounded searches: seeded in the kernel in both fleets)
        for k in robots:
            assert np.array_equal(g_on[k], g_off[k]), (what, SCENES[k], "MapGrid", which, "lists on / off")
            assert np.array_equal(g_on[k].astype(np.float64), ref_grids[k][which]), (what, SCENES[k], "MapGrid", which, "oracle")


def _results(fl):
    return [bytes(r) for r in fl.results()]


# ------------------------------------------------------------------------------------------------ one cycle
@gpu
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "whole"])
@pytest.mark.parametrize("allow_unknown", [1, 0], ids=["unknown_free", "unknown_blocked"])
@pytest.mark.parametrize("kernel", list(SIZES))
def test_lists_equal_in_kernel_seeding(nav, orc, kernel, allow_unknown, bounded):
    nx = SIZES[kernel]
    master, pos, plan_sets, ref = _reference(nav, orc, nx, allow_unknown)
    n = len(SCENES)
    on, off = _fleet(nav, nx, allow_unknown, True, bounded), _fleet(nav, nx, allow_unknown, False, bounded)
    try:
        r_on, r_off = on.find_best_path(pos, np.zeros((n, 3)), plan_sets[0]), off.find_best_path(pos, np.zeros((n, 3)), plan_sets[0])
        assert [bytes(r) for r in r_on] == [bytes(r) for r in r_off]
        boxes = on.wavefront_boxes()
        whole = [tuple(b) == (0, nx - 1, 0, NY - 1) for b in boxes]
        if bounded:
            assert whole[SCENES.index("near")] and not all(whole), ("the scenes no longer mix bounded and whole searches", boxes.tolist())
        else:
            assert all(whole)
        _compare(orc, on, off, ref[0], list(range(n)), (kernel, allow_unknown, bounded), master, plan_sets[0])
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------ capacity
@gpu
@pytest.mark.parametrize("kernel", list(SIZES))
def test_a_list_that_does_not_fit_falls_back_beside_one_that_does(nav, orc, kernel):
    """capacity 8: the path wavefronts of metre (17 cells), dense (30) and long (84) walk the plan, their goal wavefronts and
    every wavefront of the other robots (window and near: 8 cells, just fitting) use lists - in one launch"""
    nx = SIZES[kernel]
    master, pos, plan_sets, ref = _reference(nav, orc, nx, 1)
    n = len(SCENES)
    on, off = _fleet(nav, nx, 1, True, capacity=8), _fleet(nav, nx, 1, False)
    try:
        assert on.L.navgpu_planner_set_seed_list_capacity(on.h, 0) == -1 and on.L.navgpu_planner_set_seed_list_capacity(on.h, 1025) == -1
        on.find_best_path(pos, np.zeros((n, 3)), plan_sets[0])
        off.find_best_path(pos, np.zeros((n, 3)), plan_sets[0])
        assert _results(on) == _results(off)
        counts = on.seed_list_counts()
        no_list = {SCENES[k] for k in range(n) if counts[k, 0] == NO_LIST}
        assert no_list == {"metre", "dense", "long"} and (counts[:, 1:] != NO_LIST).all(), counts.tolist()
        _compare(orc, on, off, ref[0], list(range(n)), (kernel, "capacity 8"), master, plan_sets[0], capacity=8)
        # the capacity back up: the next cycle lists them all
        on.set_seed_list_capacity(1024)
        on.planner_cycle()
        assert (on.seed_list_counts() != NO_LIST).all()
        off.planner_cycle()
        _compare(orc, on, off, ref[0], list(range(n)), (kernel, "capacity 1024 again"), master, plan_sets[0])
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------ the listed cycle
@gpu
@pytest.mark.parametrize("kernel", list(SIZES))
def test_listed_cycle_with_interleaved_robots(nav, orc, kernel):
    """a whole-fleet cycle on the first plan set, then robots 0, 2, 3, 6 take the second through the listed calls: their grids are the
    second set's, the others keep the first's"""
    nx = SIZES[kernel]
    master, pos, plan_sets, ref = _reference(nav, orc, nx, 1)
    n = len(SCENES)
    listed = [0, 2, 3, 6]
    others = [k for k in range(n) if k not in listed]
    on, off = _fleet(nav, nx, 1, True), _fleet(nav, nx, 1, False)
    try:
        for fl in (on, off):
            fl.find_best_path(pos, np.zeros((n, 3)), plan_sets[0])
            fl.stage_planner_list(listed, pos[listed], np.zeros((len(listed), 3)), [plan_sets[1][k] for k in listed])
            fl.planner_cycle_list(listed)
        assert [bytes(r) for r in on.results_list(listed)] == [bytes(r) for r in off.results_list(listed)]
        mixed = [plan_sets[1][k] if k in listed else plan_sets[0][k] for k in range(n)]
        ref_mixed = [ref[1][k] if k in listed else ref[0][k] for k in range(n)]
        _compare(orc, on, off, ref_mixed, listed + others, (kernel, "listed"), master, mixed)
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------ two cycles in flight
@gpu
@pytest.mark.parametrize("kernel", list(SIZES))
def test_two_cycles_in_flight_with_a_plan_each(nav, orc, kernel):
    """two cycles queued back to back, the second with other plans: each cycle's wavefronts get the lists of their own plans"""
    from navigation_amd._lib import PlanResult
    nx = SIZES[kernel]
    master, pos, plan_sets, ref = _reference(nav, orc, nx, 1)
    n = len(SCENES)
    on, off, serial = _fleet(nav, nx, 1, True), _fleet(nav, nx, 1, False), _fleet(nav, nx, 1, False)
    try:
        got = []
        for fl in (on, off):
            fl.set_cycles_in_flight(2)
            for plans in plan_sets:
                fl.stage_planner(pos, np.zeros((n, 3)), plans)
                fl.planner_cycle()
            first = [bytes(r) for r in fl.results_previous_into((PlanResult * n)())]
            got.append((first, _results(fl)))
        assert got[0] == got[1]
        # and the first cycle's results are those of a fleet that ran it alone
        serial.find_best_path(pos, np.zeros((n, 3)), plan_sets[0])
        assert got[0][0] == _results(serial)
        _compare(orc, on, off, ref[1], list(range(n)), (kernel, "in flight"), master, plan_sets[1])
    finally:
        for fl in (on, off, serial):
            fl.close()
