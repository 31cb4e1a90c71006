"""The split image build (navgpu_planner_set_split_prep).  Needs a real MI355X.

Where k_score_sweep scores and the wavefronts run in k_bfs_rows, the grid-free part of a robot's scoring image (window bytes, footprint
screens, heading tables, aux[0..6], reject bytes) is built by extra workgroups of the wavefront launch, and k_score_prep_grids adds the
path / goal screens, the free distance (aux[7]) and start_fail (aux[8]).  With the switch off k_score_prep_tab builds the whole image
behind the wavefronts, as before.  Nothing about a result may depend on the switch, so the bar is bit equality: every case drives the
same scenario through a fleet with the split on and a twin with it off and compares every PlanResult, trajectory, sample cost and
status, oscillation record, wavefront box and level count as bytes.  The split fleet is also held against the CPU oracle, with the
comparisons tests/test_gpu_parity.py makes.

Shapes: 2 - 4 robots, maps of 48 - 130 cells per side (k_bfs_rows<7>), 6 x 5 x 7 velocity samples, 12 or 20 steps: the smallest at which
a window has several words per row, the image several table rows, and a launch more than one search and more than one prep workgroup."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwa_reference_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

RES = D.RES
BASE_CFG = dict(D.DEFAULTS, vx_samples=6, vy_samples=5, vth_samples=7, sim_time=1.2, sim_granularity=0.1, use_dwa=1, discretize_by_time=1)
MAX_PLAN = 128


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


# ------------------------------------------------------------------------------------------------ scenes
def _line(x0, y0, heading, length, start=0.0):
    d = np.arange(start, length, RES)
    return np.stack([x0 + d * np.cos(heading), y0 + d * np.sin(heading)], 1)


def _robot(kind, nx, ny, seed):
    """(master, pos, vel, plan) of one robot on an nx x ny map.  kind:
    sealed   - the plan ends inside a lethal wall: the goal grid's one seed is walled in, the robot's cell unreachable (start_fail 5)
    blocked  - the robot stands 2 cells from a lethal post (inscribed cost) and the plan starts 0.4 m ahead: its own cell is no seed and
               an obstacle in the path grid (start_fail 4)
    open     - an empty map: no screen is set anywhere in the window
    clutter  - lethal posts 0.4 - 0.9 m from the robot, inside the reach of the dilation and of some trajectories
    unknown  - clutter, and patches of NO_INFORMATION around the robot
    edge     - the robot 0.3 m from the map's left and lower border: window cells off the map
    """
    rs = np.random.RandomState(seed)
    cells = np.zeros((ny, nx), np.uint8)
    x, y, th = nx * RES * 0.3 + rs.uniform(0, 0.2), ny * RES * 0.5 + rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2)
    start, length = 0.0, min(nx * RES * 0.6, 2.4)
    if kind == "edge":
        x, y = 0.3 + rs.uniform(0, 0.05), 0.3 + rs.uniform(0, 0.05)
        th = 0.6
    cx, cy = int(x / RES), int(y / RES)
    if kind == "sealed":
        th = 0.0
        wall = min(cx + 30, nx - 3)
        cells[3:ny - 3, wall] = D.LETHAL
        length = (wall + 0.5) * RES - x + 1e-3  # the last pose lies in the wall's column
    elif kind == "blocked":
        cells[cy + 2, cx] = D.LETHAL
        start = 0.4
    elif kind in ("clutter", "unknown", "edge"):
        for _ in range(6):
            a, d = rs.uniform(0, 2 * np.pi), rs.uniform(0.4, 0.9) / RES
            px, py = int(cx + d * np.cos(a)), int(cy + d * np.sin(a))
            if 0 <= px < nx and 0 <= py < ny:
                cells[py, px] = D.LETHAL
    m = D.inflate(cells)
    if kind == "unknown":
        for _ in range(4):
            a, d = rs.uniform(0, 2 * np.pi), rs.uniform(0.3, 0.8) / RES
            px, py = int(cx + d * np.cos(a)), int(cy + d * np.sin(a))
            m[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = D.NOINFO
    pos = np.array([x, y, th], np.float32)
    vel = np.array([rs.uniform(0.1, 0.4), 0.0, rs.uniform(-0.3, 0.3)], np.float32)
    plan = _line(float(pos[0]), float(pos[1]), th + (0.0 if kind == "sealed" else rs.uniform(-0.15, 0.15)), length, start)
    assert 1 <= len(plan) <= MAX_PLAN
    return m, pos, vel, plan


_SCENES = {}


def _scene(kinds, nx, ny):
    """one robot per entry of kinds; computed once and left unchanged"""
    key = (tuple(kinds), nx, ny)
    if key not in _SCENES:
        robots = [_robot(k, nx, ny, 100 * i + nx) for i, k in enumerate(kinds)]
        for r in robots:
            r[0].setflags(write=False)
        _SCENES[key] = robots
    return _SCENES[key]


def _fleet(nav, robots, nx, ny, cfg, split, fp=D.FP4):
    from navigation_amd import _lib as N
    fl = nav.Fleet(len(robots), nx, ny, RES, layers=N.LAYER_OBSTACLE, keep_sample_costs=True, max_sim_steps=32, max_plan=MAX_PLAN)
    fl.configure_planner(nav.DwaConfig(**cfg))
    fl.set_footprint(fp)
    fl.upload(N.GRID_MASTER, np.stack([r[0] for r in robots]))
    fl.set_split_prep(split)
    fl.set_plan()
    return fl


def _state(fl, i):
    """what a cycle leaves for robot i, as bytes"""
    flags, prev = fl.oscillation(i, 1)
    return dict(result=bytes(fl.results(i, 1)[0]), trajectory=fl.trajectory(i).tobytes(), samples=b"".join(a.tobytes() for a in fl.samples(i)),
                oscillation=flags.tobytes() + prev.tobytes(), box=fl.wavefront_boxes(i, 1).tobytes(), levels=fl.wavefront_levels(i, 1).tobytes())


def _assert_same(fa, fb, robots, what):
    for i in robots:
        a, b = _state(fa, i), _state(fb, i)
        for k in a:
            assert a[k] == b[k], (what, "robot", i, k)


def _oracle_planners(orc, nav, robots, cfg):
    ocfg = orc.DwaConfig(**nav.DwaConfig(**cfg).as_dict())
    ps = [orc.DwaPlanner(r[0], RES, 0.0, 0.0, ocfg) for r in robots]
    for p in ps:
        p.set_plan()
    return ps


def _assert_oracle(fl, k, p, pos, vel, plan, fp, what):
    """tests/test_gpu_parity.py's comparisons of a robot's cycle with the oracle's; returns the oracle's result"""
    ores, otraj, _, cfull, ostatus = p.cycle(pos, vel, plan, fp)
    r = fl.results(k, 1)[0]
    cost, status, vels = fl.samples(k)
    assert len(cost) == ores.n_samples == r.n_samples, what
    assert np.array_equal(vels.view(np.uint32), p.samples().view(np.uint32)), what
    assert np.array_equal(status, ostatus), what
    scored = status == 1
    neg_o, neg_g = cfull[scored] < 0, cost[scored] < 0
    assert np.array_equal(neg_o, neg_g), (what, "valid / invalid mask")
    assert np.array_equal(cfull[scored][neg_o], cost[scored][neg_g]), (what, "failure codes")
    assert np.allclose(cost[scored][~neg_g], cfull[scored][~neg_o], rtol=0, atol=1e-5), what
    assert r.best_index == ores.best_index and r.n_scored == ores.n_scored and r.n_valid == ores.n_valid, what
    assert abs(r.cost - ores.cost) <= 1e-5 and r.oscillation_flags == ores.oscillation_flags, what
    if r.best_index >= 0:
        assert (r.xv, r.yv, r.thetav) == (ores.xv, ores.yv, ores.thetav), what
        t = fl.trajectory(k)
        assert t.shape == otraj.shape and np.allclose(t, otraj, rtol=0, atol=1e-6), what
    return ores


def _twins(nav, orc, kinds, nx, ny, cfg=None, fp=D.FP4, cycles=2):
    """the scene through a split fleet and its twin, `cycles` cycles (the pose moves, the velocity turns); returns the oracle's results of the last"""
    cfg = dict(BASE_CFG, **(cfg or {}))
    robots = _scene(kinds, nx, ny)
    A, B = _fleet(nav, robots, nx, ny, cfg, True, fp), _fleet(nav, robots, nx, ny, cfg, False, fp)
    planners = _oracle_planners(orc, nav, robots, cfg)
    try:
        for cyc in range(cycles):
            pos = np.stack([r[1] for r in robots]).copy()
            vel = np.stack([r[2] for r in robots]).copy()
            pos[:, 0] += 0.03 * cyc
            pos[:, 2] += 0.3 * cyc
            if cyc & 1:
                vel[:, 2] = -vel[:, 2]
            plans = [r[3] for r in robots]
            for fl in (A, B):
                fl.find_best_path(pos, vel, plans)
            _assert_same(A, B, range(len(robots)), (kinds, nx, ny, "cycle", cyc))
            ores = [_assert_oracle(A, k, planners[k], pos[k], vel[k], plans[k], fp, (kinds, nx, ny, "cycle", cyc, "robot", k)) for k in range(len(robots))]
        return ores
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ a. start_fail, the free distance
def test_goal_sealed_in_a_wall(nav, orc):
    ores = _twins(nav, orc, ("sealed", "sealed"), 96, 80)
    assert all(o.n_scored > 0 and o.n_valid == 0 for o in ores), "the goal critic fails every sample of a robot whose goal is walled in"


def test_own_cell_blocked_in_the_path_grid(nav, orc):
    ores = _twins(nav, orc, ("blocked", "blocked"), 96, 80)
    assert all(o.n_scored > 0 and o.n_valid == 0 for o in ores), "the path critic fails every sample of a robot on a blocked cell"


def test_both_beside_an_ordinary_robot(nav, orc):
    ores = _twins(nav, orc, ("sealed", "blocked", "clutter", "open"), 96, 80)
    assert [o.n_valid > 0 for o in ores] == [False, False, True, True]


def test_open_ground(nav, orc):
    ores = _twins(nav, orc, ("open", "open"), 130, 130)
    assert all(o.n_valid == o.n_scored > 0 for o in ores)


def test_clutter_inside_the_disc(nav, orc):
    ores = _twins(nav, orc, ("clutter", "clutter", "clutter"), 130, 96)
    assert any(0 < o.n_valid < o.n_scored for o in ores), "no robot has both legal and colliding samples: the scene tells nothing"


# ------------------------------------------------------------------------------------------------ b. off-map and off-window cells
def test_robot_at_the_map_edge(nav, orc):
    _twins(nav, orc, ("edge", "clutter"), 130, 64)


def test_map_smaller_than_the_window(nav, orc):
    """20 steps of 0.1 s at 0.55 m / s and the footprint reach beyond 24 cells either way: the window is wider than the 48-cell map"""
    _twins(nav, orc, ("clutter", "edge"), 48, 48, cfg=dict(sim_time=2.0))


# ------------------------------------------------------------------------------------------------ c. configurations
@pytest.mark.parametrize("cfg", [dict(allow_unknown=0), dict(allow_unknown=1), dict(sum_scores=1), dict(rollout_trig=1), dict(path_distance_bias=0.0),
                                 dict(goal_distance_bias=0.0)], ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_configurations(nav, orc, cfg):
    _twins(nav, orc, ("unknown", "clutter", "sealed"), 112, 80, cfg=cfg)


def test_nine_vertex_footprint(nav, orc):
    _twins(nav, orc, ("clutter", "unknown"), 96, 96, fp=D.FP9)


# ------------------------------------------------------------------------------------------------ d. two cycles in flight, one image buffer
def test_two_cycles_in_flight(nav, orc):
    """four cycles with a new costmap, pose and velocity each: the split fleet queues cycle k + 1 before it reads cycle k, its twin runs
    one cycle at a time with the split off"""
    from navigation_amd import _lib as N
    kinds, nx, ny, n_cyc = ("clutter", "sealed", "unknown", "blocked"), 112, 80, 4
    robots = _scene(kinds, nx, ny)
    n = len(robots)
    A, B = _fleet(nav, robots, nx, ny, BASE_CFG, True), _fleet(nav, robots, nx, ny, BASE_CFG, False)
    try:
        A.set_cycles_in_flight(2)
        plans = [r[3] for r in robots]
        got, want = [], []
        buf = (N.PlanResult * n)()
        for cyc in range(n_cyc):
            masters = np.stack([r[0] for r in robots]).copy()
            masters[:, 4 + cyc, 4:12] = D.LETHAL  # (the changed scan)
            pos = np.stack([r[1] for r in robots]).copy()
            vel = np.stack([r[2] for r in robots]).copy()
            pos[:, 0] += 0.04 * cyc
            pos[:, 2] -= 0.2 * cyc
            vel[:, 0] += 0.02 * cyc
            for fl in (A, B):
                fl.upload(N.GRID_MASTER, masters)
                fl.stage_planner(pos, vel, plans)
                fl.planner_cycle()
            if cyc:
                got.append([bytes(r) for r in A.results_previous_into(buf)])
            want.append([bytes(r) for r in B.results()])
        got.append([bytes(r) for r in A.results()])
        assert got == want
        _assert_same(A, B, range(n), "after the last cycle")
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ e. the listed cycle
def test_listed_cycle_skips_robots(nav, orc):
    kinds, nx, ny = ("clutter", "sealed", "unknown", "blocked"), 112, 80
    robots = _scene(kinds, nx, ny)
    listed, others = [0, 2, 3], [1]
    A, B = _fleet(nav, robots, nx, ny, BASE_CFG, True), _fleet(nav, robots, nx, ny, BASE_CFG, False)
    try:
        pos, vel, plans = np.stack([r[1] for r in robots]), np.stack([r[2] for r in robots]), [r[3] for r in robots]
        for fl in (A, B):
            fl.find_best_path(pos, vel, plans)
        before = {i: _state(A, i) for i in others}
        pos2 = pos[listed].copy()
        pos2[:, 0] += 0.05
        pos2[:, 2] += 0.25
        for fl in (A, B):
            fl.stage_poses_list(listed, pos2, vel[listed])
            fl.planner_cycle_list(listed)
        _assert_same(A, B, range(len(robots)), "listed cycle")
        for i in others:
            assert _state(A, i) == before[i], ("unlisted robot", i)
        planners = _oracle_planners(orc, nav, robots, BASE_CFG)
        for k, i in enumerate(listed):
            planners[i].cycle(pos[i], vel[i], plans[i], D.FP4)  # (the cycle before: the oscillation record)
            _assert_oracle(A, i, planners[i], pos2[k], vel[i], plans[i], D.FP4, ("listed cycle", i))
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ f. maps of the other wavefront kernels
@pytest.mark.parametrize("nx,ny", [(672, 48), (1056, 48)], ids=["k_bfs_rows2", "k_bfs_global"])
def test_other_wavefront_kernels_build_the_image_whole(nav, orc, nx, ny):
    """21 and 33 words per row: not k_bfs_rows' maps, the switch changes nothing about the launches"""
    _twins(nav, orc, ("clutter", "edge"), nx, ny, cycles=1)


# ------------------------------------------------------------------------------------------------ g. the switch between cycles
def test_switching_between_cycles(nav, orc):
    kinds, nx, ny = ("clutter", "sealed", "blocked"), 96, 80
    robots = _scene(kinds, nx, ny)
    A, B = _fleet(nav, robots, nx, ny, BASE_CFG, True), _fleet(nav, robots, nx, ny, BASE_CFG, False)
    planners = _oracle_planners(orc, nav, robots, BASE_CFG)
    try:
        plans = [r[3] for r in robots]
        for cyc, split in enumerate((True, False, True, True, False)):
            A.set_split_prep(split)
            pos = np.stack([r[1] for r in robots]).copy()
            vel = np.stack([r[2] for r in robots]).copy()
            pos[:, 1] += 0.03 * cyc
            pos[:, 2] += 0.15 * cyc
            for fl in (A, B):
                fl.find_best_path(pos, vel, plans)
            _assert_same(A, B, range(len(robots)), ("cycle", cyc, "split", split))
            for k in range(len(robots)):
                _assert_oracle(A, k, planners[k], pos[k], vel[k], plans[k], D.FP4, ("cycle", cyc, "robot", k))
    finally:
        A.close()
        B.close()
