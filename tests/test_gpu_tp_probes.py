"""navgpu_tp_score_trajectories (k_tp_probe: a wave per probe, a lane per step) and navgpu_tp_update_plans.  Need a real MI355X.

1. Against the reference: every `pre` / `post` probe of every case of tests/golden/g16_tp_reference.npz, one batched call per cycle, as a
   fleet of one and as robot 1 of 3 with flipped maps.  Bar of tests/test_gpu_tp_reference.py: codes equal, costs within relative 1e-9,
   ok equal.
2. Against the serial kernel of the same build (navgpu_tp_score_trajectory: one lane of k_tp_rollout): == on the doubles, at the shapes
   where a lane per step can go wrong.  The serial calls are made before and after the batched one.
3. navgpu_tp_update_plans over a range against a twin fleet fed by single navgpu_tp_update_plan calls: the grids' bytes."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tp_reference_cases as T  # noqa: E402
from tp_reference_cases import FP2, FP4, INSCRIBED, LETHAL, NOINFO, RES, line  # noqa: E402

pytestmark = pytest.mark.gpu

G, META = T.load()
COST_RTOL = 1e-9
STEPS = 160  # max_sim_steps of the fleets here: above the 136 steps of the halved granularity


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _same_cost(got, want):
    return got == want if want < 0 else (got >= 0 and abs(got - want) <= COST_RTOL * max(1.0, abs(want)))


def _probes(pos, vel, samples):
    s = np.asarray(samples, np.float64).reshape(-1, 3)
    return np.concatenate([np.tile(np.concatenate([np.asarray(pos, np.float64), np.asarray(vel, np.float64)]), (len(s), 1)), s], axis=1)


# ------------------------------------------------------------------------------------------------ 1. against the reference
def _run_reference(nav, name, n_inst, robot):
    from navigation_amd import _lib as N
    c, costmap, cycles = T.case(G, META, name)
    maps = [costmap] * n_inst
    if n_inst > 1:
        maps = [np.ascontiguousarray(costmap[::-1]), costmap, np.ascontiguousarray(costmap[:, ::-1])]
    fl = nav.Fleet(n_inst, c["size_x"], c["size_y"], c["res"], layers=N.LAYER_OBSTACLE, max_sim_steps=max(c["max_sim_steps"], 80), max_plan=256)
    try:
        fl.set_origin(np.array([c["origin"]] * n_inst))
        fl.set_footprint(c["fp"])
        fl.upload(N.GRID_MASTER, np.stack(maps))
        configured = False
        checked = 0
        for k, cyc in enumerate(cycles):
            where = f"{name} cycle {k} robot {robot} of {n_inst}"
            if not configured or cyc.reconfigure:
                kw = {key: v for key, v in cyc.cfg.items() if key != "meter_scoring"}
                fl.configure_trajectory_planner(N.TpConfig(allow_unknown=c["allow_unknown"], **kw))
                configured = True
            if cyc.plan is not None:
                fl.tp_update_plans([cyc.plan] * n_inst, compute_dists=bool(cyc.compute_dists))
            pos64, vel64 = cyc.pos.astype(np.float64), cyc.vel.astype(np.float64)
            everyone = list(range(n_inst))  # every robot carries the probes; the one under test is read
            if len(cyc.pre_samples):
                run = _probes(pos64, vel64, cyc.pre_samples)
                costs, ok = fl.tp_score_trajectories(everyone, [run] * n_inst)
                got = costs.reshape(n_inst, -1)[robot]
                for s, g, want in zip(cyc.pre_samples, got, cyc.pre):
                    print(f"{where}: scoreTrajectory{tuple(s)} before findBestPath {g!r} reference {want!r}")
                    assert _same_cost(g, want), where
                    checked += 1
                assert np.array_equal(ok, costs >= 0)
            fl.tp_find_best_path(np.stack([cyc.pos] * n_inst), np.stack([cyc.vel] * n_inst))
            if len(cyc.post_samples):
                run = _probes(pos64, vel64, cyc.post_samples)
                costs, ok = fl.tp_score_trajectories(everyone, [run] * n_inst)
                got, got_ok = costs.reshape(n_inst, -1)[robot], ok.reshape(n_inst, -1)[robot]
                for s, g, o, (want_cost, want_ok) in zip(cyc.post_samples, got, got_ok, cyc.post):
                    print(f"{where}: scoreTrajectory{tuple(s)} after findBestPath {g!r} reference {want_cost!r}")
                    assert _same_cost(g, want_cost) and bool(o) == bool(want_ok) == (g >= 0), (where, tuple(s), g, want_cost)
                    checked += 1
        return checked
    finally:
        fl.close()


@pytest.mark.parametrize("name", META["cases"])
def test_reference_probes_fleet_of_one(nav, name):
    _run_reference(nav, name, 1, 0)


@pytest.mark.parametrize("name", META["cases"])
def test_reference_probes_robot_1_of_three(nav, name):
    _run_reference(nav, name, 3, 1)


def test_the_fixture_holds_probes():
    n = sum(len(cyc.pre_samples) + len(cyc.post_samples) for name in META["cases"] for cyc in T.case(G, META, name)[2])
    assert n >= 40, n


# ------------------------------------------------------------------------------------------------ 2. against the serial kernel
NX = NY = 64
X0, Y0 = 0.51, 1.62          # where the eastbound probes start: cell (10, 32), not on a cell border
WALL, BAND, NEAR_WALL, SPOT = 45, 30, 36, (26, 35)  # cell columns / one cell, see _maps
BASE = dict(sim_time=1.7, sim_granularity=0.025, angular_sim_granularity=0.025, max_vel_x=1.0, max_vel_th=2.0, min_vel_th=-2.0, vx_samples=3,
            vtheta_samples=3)


def _num_steps(cfg, vs):  # trajectory_planner.cpp:236-249
    if cfg.get("heading_scoring"):
        return max(1, int(cfg["sim_time"] / cfg["sim_granularity"] + 0.5))
    return max(1, int(max(math.hypot(vs[0], vs[1]) * cfg["sim_time"] / cfg["sim_granularity"], abs(vs[2]) / cfg["angular_sim_granularity"]) + 0.5))


def _maps():
    """Five robots, five maps (rows are y, columns x; 0.05 m cells, origin 0, 0).
    0: a lethal wall over every row of column WALL.  An eastbound probe at 1 m/s from X0 (68 steps of 0.025 m) brings its front edge
       (0.15 m ahead) into the wall at step 64: a failure in the second chunk only.
    1: an INSCRIBED band at column BAND (the footprint's outline passes it, the MapGrids call it an obstacle: -2 when the centre enters,
       step 40) and a lethal wall at column NEAR_WALL (-1 when the front edge arrives, step 46): -2, then -1.
    2: one lethal cell SPOT on the row of the footprint's upper edge (-1 from step 26 on) and the same band (-2 at step 40): -1, then -2.
    3: a block of NO_INFORMATION on the way.
    4: a lethal wall between the robot and the far part of its plan (heading scoring: the line of sight)."""
    m = [np.zeros((NY, NX), np.uint8) for _ in range(5)]
    m[0][:, WALL] = LETHAL
    m[1][:, BAND] = INSCRIBED
    m[1][:, NEAR_WALL] = LETHAL
    m[2][SPOT[1], SPOT[0]] = LETHAL
    m[2][:, BAND] = INSCRIBED
    m[3][28:37, 40:45] = NOINFO
    m[4][16:48, 30] = LETHAL
    return m


EAST = line((X0, Y0), (2.0, Y0))
PLANS = [EAST, line((X0, Y0), (1.2, Y0)), line((X0, Y0), (1.2, Y0)), EAST,
         np.concatenate([line((X0, Y0), (X0, 2.8)), line((X0 + 0.05, 2.8), (2.6, 2.8)), line((2.6, 2.75), (2.6, Y0))])]
V64, V65 = 64 * 0.025 / 1.7, 65 * 0.025 / 1.7
START, MOVING = (X0, Y0, 0.0), (1.0, 0.0, 0.0)  # already at 1 m/s: the eastbound steps are 0.025 m from the first on
NORTH = (0.61, 0.41, math.pi / 2)


@pytest.fixture(scope="module")
def five(nav):
    from navigation_amd import _lib as N
    fl = nav.Fleet(5, NX, NY, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=STEPS, max_plan=256)
    fl.set_origin(np.zeros((5, 2)))
    fl.upload(N.GRID_MASTER, np.stack(_maps()))
    yield fl
    fl.close()


def _setup(fl, fp=FP4, **kw):
    """configure, plans with their grids, one findBestPath (the `last cycle` the batched call must leave alone)"""
    from navigation_amd import _lib as N
    cfg = dict(BASE)
    cfg.update(kw)
    fl.set_footprint(np.asarray(fp, np.float64))
    fl.configure_trajectory_planner(N.TpConfig(**cfg))
    fl.tp_update_plans(PLANS, compute_dists=True)
    fl.tp_find_best_path(np.tile(np.asarray(START, np.float32), (5, 1)), np.zeros((5, 3), np.float32))
    return cfg


def _compare(fl, instances, runs):
    """serial, batched, serial again: the same doubles; the last cycle's samples and trajectory untouched by the batched call"""
    last = [(fl.tp_samples(i), fl.tp_trajectory(i)) for i in range(fl.n)]
    serial = lambda: np.array([fl.tp_score_trajectory(i, p[0:3], p[3:6], p[6:9]) for i, run in zip(instances, runs) for p in run])  # noqa: E731
    before = serial()
    costs, ok = fl.tp_score_trajectories(instances, runs)
    for i, (samples, traj) in enumerate(last):
        assert fl.tp_samples(i) == samples and np.array_equal(fl.tp_trajectory(i), traj), f"robot {i}: the last cycle moved"
    after = serial()
    for q, (b, g, a) in enumerate(zip(before, costs, after)):
        print(f"probe {q}: serial {b!r} batched {g!r} serial again {a!r}")
    assert len(costs) == sum(len(r) for r in runs)
    assert np.array_equal(before, costs) and np.array_equal(after, costs), (before, costs, after)
    assert np.array_equal(ok, costs >= 0)
    return costs


def test_step_counts_and_chunks(five):
    """0 -> 1 step, exactly 64, 65, 68 steps; a failure in the second chunk only; a trajectory that leaves the map; several probes per
    robot, a listed robot without probes, instances 0, 2, 4 of 5"""
    cfg = _setup(five)
    samples = [(0.0, 0.0, 0.0), (V64, 0.0, 0.0), (V65, 0.0, 0.0), (0.0, 0.0, 1.625), (1.0, 0.0, 0.0), (0.3, 0.1, -0.7)]
    assert [_num_steps(cfg, s) for s in samples] == [1, 64, 65, 65, 68, 28]
    north = _probes(NORTH, (0, 0, 0), samples)
    # eastbound at 1 m/s: step i stands at X0 + 0.025 i, its front edge 0.15 m ahead; the wall begins at WALL * RES
    assert X0 + 0.025 * 63 + 0.15 < WALL * RES - 0.005 and X0 + 0.025 * 64 + 0.15 > WALL * RES + 0.005
    # 68 steps into the wall at step 64; the same 68 steps begun 0.1 m (4 steps) earlier stay clear of it, so none of the steps 0 .. 63
    # of the first fails: the -1 comes from the second chunk
    east = _probes(START, MOVING, [(1.0, 0.0, 0.0)])
    earlier = _probes((X0 - 0.1, Y0, 0.0), MOVING, [(1.0, 0.0, 0.0)])
    leaves = _probes((2.9, 0.6, 0.0), MOVING, [(1.0, 0.0, 0.0)])  # on robot 4's map: its east is connected to its plan
    costs = _compare(five, [0, 2, 4], [np.concatenate([north, east, earlier]), np.zeros((0, 9)), np.concatenate([north[:3], leaves])])
    assert (costs[:6] >= 0).all() and (costs[8:11] >= 0).all(), costs  # open floor
    assert costs[6] == -1.0 and costs[7] >= 0, costs                    # the wall, in the second chunk only
    assert costs[11] == -1.0, costs                                     # off the map


def test_first_failure_wins(five):
    """-2 at step 40, -1 at step 46 (robot 1); -1 at step 26, -2 at step 40 (robot 2): both failures of a pair lie in chunk 0, the lower
    step's code is the answer"""
    _setup(five)
    assert X0 + 0.025 * 39 < BAND * RES < X0 + 0.025 * 40 and X0 + 0.025 * 45 + 0.15 < NEAR_WALL * RES < X0 + 0.025 * 46 + 0.15
    assert X0 + 0.025 * 25 + 0.15 < SPOT[0] * RES < X0 + 0.025 * 26 + 0.15 and SPOT[1] == int((Y0 + 0.15) / RES)
    fast = _probes(START, MOVING, [(1.0, 0.0, 0.0)])
    slow = _probes(START, (0.5, 0.0, 0.0), [(0.5, 0.0, 0.0)])  # 34 steps over 0.85 m: ends before either obstacle of robot 1
    costs = _compare(five, [1, 2], [np.concatenate([fast, slow]), np.concatenate([fast, slow])])
    assert costs[0] == -2.0 and costs[1] >= 0, costs   # robot 1: the band comes first
    assert costs[2] == -1.0 and costs[3] == -1.0, costs  # robot 2: the lethal cell comes first (the slow probe reaches it too)
    # the later failure alone gives the other code: robot 1 without the band fails with -1, robot 2 without the spot with -2
    from navigation_amd import _lib as N
    m = _maps()
    m[1][:, BAND] = 0
    m[2][SPOT[1], SPOT[0]] = 0
    five.upload(N.GRID_MASTER, np.stack(m))
    try:
        five.tp_update_plans(PLANS, compute_dists=True)
        costs = _compare(five, [1, 2], [fast, fast])
        assert costs[0] == -1.0 and costs[1] == -2.0, costs
    finally:
        five.upload(N.GRID_MASTER, np.stack(_maps()))


def test_first_failure_across_chunks(five):
    """With half the granularity the 1 m/s probe has 136 steps of 0.0125 m, three chunks.  Robot 1, begun at x = 0.81: the band at step 56
    (chunk 0), the wall at step 68 (chunk 1).  Robot 2, begun at X0: the lethal cell at step 52 (chunk 0), the band at step 80 (chunk 1).
    The chunk behind the first failure is not evaluated, and its failure must not show."""
    cfg = _setup(five, sim_granularity=0.0125)
    assert _num_steps(cfg, (1.0, 0.0, 0.0)) == 136
    assert 0.81 + 0.0125 * 55 < BAND * RES < 0.81 + 0.0125 * 56 < 0.81 + 0.0125 * 63
    assert 0.81 + 0.0125 * 67 + 0.15 < NEAR_WALL * RES < 0.81 + 0.0125 * 68 + 0.15
    assert X0 + 0.0125 * 51 + 0.15 < SPOT[0] * RES < X0 + 0.0125 * 52 + 0.15 and X0 + 0.0125 * 79 < BAND * RES < X0 + 0.0125 * 80
    fast = _probes(START, MOVING, [(1.0, 0.0, 0.0)])
    costs = _compare(five, [1, 2], [_probes((0.81, Y0, 0.0), MOVING, [(1.0, 0.0, 0.0)]), fast])
    assert costs[0] == -2.0 and costs[1] == -1.0, costs


def test_heading_scoring(five):
    """heading_scoring: 68 steps whatever the sample, headingDiff on the one step in the window; robot 0 sees its plan, robot 4's plan lies
    behind a wall but for its first leg"""
    cfg = _setup(five, heading_scoring=1, heading_scoring_timestep=0.1)
    assert _num_steps(cfg, (0.2, 0.0, 0.1)) == 68
    run = _probes(START, (0.2, 0.0, 0.0), [(0.3, 0.0, 0.2), (0.0, 0.0, -0.8), (0.2, 0.1, 0.0)])
    costs = _compare(five, [0, 4], [run, run])
    assert (costs >= 0).all() and not np.array_equal(costs[:3], costs[3:]), costs
    # a window no step falls into: heading_diff stays 0, the distances are never taken
    _setup(five, heading_scoring=1, heading_scoring_timestep=5.0)
    costs = _compare(five, [0, 4], [run, run])
    assert (costs >= 0).all()
    # nothing of the plan in sight (robot 4, a plan wholly behind the wall): DBL_MAX goes into the cost
    _setup(five, heading_scoring=1, heading_scoring_timestep=0.1)
    five.tp_update_plan(4, line((2.6, 2.0), (2.6, 1.2)), compute_dists=True)
    costs = _compare(five, [4], [run])
    assert (costs > 1e300).all(), costs


def test_simple_attractor_footprint_of_two_and_unknown_cells(five):
    from navigation_amd import _lib as N
    run = _probes(START, MOVING, [(1.0, 0.0, 0.0), (0.4, 0.0, 0.3), (0.0, 0.0, 0.0)])
    _setup(five, simple_attractor=1)
    costs = _compare(five, [0, 1, 3], [run, run, run])
    assert costs[0] == -1.0 and costs[1] >= 0 and costs[3] == -1.0 and costs[6] >= 0, costs  # no -2 without the grids: robot 1 runs into its wall
    five.tp_update_plan(2, np.zeros((0, 2)))
    with pytest.raises(N.NavgpuError, match=r"\(-5\)"):  # simple_attractor indexes the plan's last pose
        five.tp_score_trajectories([1, 2], [run, run])
    assert len(five.tp_score_trajectories([1, 2], [run, np.zeros((0, 9))])[0]) == 3  # a robot without probes is left alone
    # a 2-vertex footprint is the centre cell alone, and INSCRIBED fails there
    _setup(five, fp=FP2)
    costs = _compare(five, [0, 1], [run, run])
    assert costs[0] >= 0 and costs[3] == -1.0, costs  # robot 0's centre never reaches its wall; robot 1's enters the band
    # NO_INFORMATION under the outline: legal (and dear) with allow_unknown, -1 without
    _setup(five, allow_unknown=1)
    with_unknown = _compare(five, [3], [run])
    _setup(five, allow_unknown=0)
    without = _compare(five, [3], [run])
    assert with_unknown[0] >= 0 and without[0] == -1.0 and with_unknown[2] >= 0 and without[2] >= 0, (with_unknown, without)


def test_lists_and_errors(nav, five):
    from navigation_amd import _lib as N
    _setup(five)
    costs, ok = five.tp_score_trajectories([], [])
    assert len(costs) == 0 and len(ok) == 0
    costs, ok = five.tp_score_trajectories([1, 3], [np.zeros((0, 9)), np.zeros((0, 9))])
    assert len(costs) == 0
    run = _probes(START, MOVING, [(1.0, 0.0, 0.0)])
    for bad in (np.nan, np.inf):
        p = run.copy()
        p[0, 7] = bad
        with pytest.raises(N.NavgpuError, match=r"\(-1\)"):
            five.tp_score_trajectories([0], [p])
    for inst in ([2, 1], [1, 1], [1, 5]):
        with pytest.raises(N.NavgpuError, match=r"\(-1\)"):
            five.tp_score_trajectories(inst, [run, run])
    with pytest.raises(N.NavgpuError, match=r"\(-4\)"):  # a plan that does not fit: nothing changes for any robot
        five.tp_update_plans([EAST, np.zeros((257, 2))], compute_dists=True, first=3)
    fresh = nav.Fleet(2, NX, NY, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=STEPS, max_plan=256)
    try:
        with pytest.raises(N.NavgpuError, match=r"\(-5\)"):  # before navgpu_tp_configure
            fresh.tp_score_trajectories([0], [run])
        with pytest.raises(N.NavgpuError, match=r"\(-5\)"):
            fresh.tp_update_plans([EAST, EAST])
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 3. navgpu_tp_update_plans
@pytest.mark.parametrize("compute_dists", [True, False])
def test_update_plans_equals_single_calls(nav, five, compute_dists):
    from navigation_amd import _lib as N
    _setup(five)
    twin = nav.Fleet(5, NX, NY, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=STEPS, max_plan=256)
    try:
        twin.set_origin(np.zeros((5, 2)))
        twin.upload(N.GRID_MASTER, np.stack(_maps()))
        twin.set_footprint(np.asarray(FP4, np.float64))
        twin.configure_trajectory_planner(N.TpConfig(**BASE))
        for i, p in enumerate(PLANS):
            twin.tp_update_plan(i, p, compute_dists=True)
        twin.tp_find_best_path(np.tile(np.asarray(START, np.float32), (5, 1)), np.zeros((5, 3), np.float32))  # as _setup does
        # new plans for robots 1 .. 3 (one of them empty); 0 and 4 keep theirs
        new = [line((2.0, 0.5), (0.4, 0.5)), np.zeros((0, 2)), line((X0, Y0), (X0, 2.9))]
        five.tp_update_plans(new, compute_dists=compute_dists, first=1)
        for i, p in enumerate(new):
            twin.tp_update_plan(1 + i, p, compute_dists=compute_dists)
        for gid in (N.GRID_PATH, N.GRID_GOAL):
            assert np.array_equal(five.download(gid), twin.download(gid)), (gid, compute_dists)
        # the host side took the plans either way: findBestPath uploads them and answers alike
        pos, vel = np.tile(np.asarray(START, np.float32), (5, 1)), np.zeros((5, 3), np.float32)
        a, b = five.tp_find_best_path(pos, vel), twin.tp_find_best_path(pos, vel)
        assert [bytes(x) for x in a] == [bytes(x) for x in b]
        for gid in (N.GRID_PATH, N.GRID_GOAL):
            assert np.array_equal(five.download(gid), twin.download(gid)), (gid, compute_dists)
    finally:
        twin.close()
