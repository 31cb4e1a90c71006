"""The legacy TrajectoryPlanner on the device (k_tp_within, the MapGrid wavefronts with within_robot, k_tp_rollout, the host replay of
createTrajectories' selection in navgpu_tp.cpp) against the reference's own numbers: tests/golden/g16_tp_reference.npz, written by
tools/make_tp_goldens.py from base_local_planner::TrajectoryPlanner compiled in place.  Reads the fixture only: no reference tree, no
CPU oracle.  Need a real MI355X.

Bar (that of tests/test_gpu_parity.py::_tp_compare_cycle): grids, call count, sample velocities, legal / illegal mask, failure codes,
lengths, winner velocities, best_sample, n_points, flags and the five state doubles equal; costs within relative 1e-9; trajectory
points within 1e-12; drive x and y equal, drive yaw within DRIVE_YAW_BOUND (the reference hands it back through a quaternion)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tp_reference_cases as T  # noqa: E402
from test_dwa_reference import DRIVE_YAW_BOUND  # noqa: E402

pytestmark = pytest.mark.gpu

G, META = T.load()
COST_RTOL, POINT_ATOL = 1e-9, 1e-12


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _same_cost(got, want):
    return got == want if want < 0 else (got >= 0 and abs(got - want) <= COST_RTOL * max(1.0, abs(want)))


def _run(nav, name, n_inst, robot, other_allow_unknown=False):
    from navigation_amd import _lib as N
    c, costmap, cycles = T.case(G, META, name)
    if other_allow_unknown:  # no map holds unknown cells: the reference gives the same record for both values (meta)
        c["allow_unknown"] = 1 - c["allow_unknown"]
    maps = [costmap] * n_inst
    if n_inst > 1:  # the other robots carry other maps of the same size: batch indexing
        maps = [np.ascontiguousarray(costmap[::-1]), costmap, np.ascontiguousarray(costmap[:, ::-1])]
        assert not np.array_equal(maps[0], costmap) and not np.array_equal(maps[2], costmap)
    fl = nav.Fleet(n_inst, c["size_x"], c["size_y"], c["res"], layers=N.LAYER_OBSTACLE, max_sim_steps=c["max_sim_steps"], max_plan=256)
    try:
        fl.set_origin(np.array([c["origin"]] * n_inst))
        fl.set_footprint(c["fp"])
        fl.upload(N.GRID_MASTER, np.stack(maps))
        configured = False
        for k, cyc in enumerate(cycles):
            where = f"{name} cycle {k} robot {robot} of {n_inst} allow_unknown {c['allow_unknown']}"
            if not configured or cyc.reconfigure:  # the scales are the reference's own, after meter_scoring
                kw = {key: v for key, v in cyc.cfg.items() if key != "meter_scoring"}
                fl.configure_trajectory_planner(N.TpConfig(allow_unknown=c["allow_unknown"], **kw))
                configured = True
            if cyc.plan is not None:
                for r in range(n_inst):
                    fl.tp_update_plan(r, cyc.plan, compute_dists=bool(cyc.compute_dists))
            pos64, vel64 = cyc.pos.astype(np.float64), cyc.vel.astype(np.float64)
            for s, want in zip(cyc.pre_samples, cyc.pre):  # updatePlan(compute_dists = true), then scoreTrajectory
                got = fl.tp_score_trajectory(robot, pos64, vel64, s)
                print(f"{where}: scoreTrajectory{tuple(s)} before findBestPath {got!r} reference {want!r}")
                assert _same_cost(got, want), where
            r = fl.tp_find_best_path(np.stack([cyc.pos] * n_inst), np.stack([cyc.vel] * n_inst))[robot]
            for gid, which in ((N.GRID_PATH, 0), (N.GRID_GOAL, 1)):
                got = fl.download(gid, robot, 1)[0]
                assert np.array_equal(got.astype(np.float64), cyc.grid[which].astype(np.float64)), f"{where}: MapGrid {which}"
            calls = np.asarray(fl.tp_samples(robot), np.float64).reshape(-1, 5)
            want = cyc.calls
            assert len(calls) == len(want) == r.n_samples, (where, len(calls), len(want), r.n_samples)
            assert np.array_equal(calls[:, :3], want[:, :3]), f"{where}: sample velocities"
            ok = want[:, 3] >= 0
            d = np.abs(calls[ok, 3] - want[ok, 3]) / np.maximum(1.0, np.abs(want[ok, 3])) if np.array_equal(calls[:, 3] >= 0, ok) else np.array([np.nan])
            print(f"{where}: calls {len(want)} legal {int(ok.sum())} max relative |cost - reference| {d.max(initial=0.0):.3e}")
            assert np.array_equal(calls[:, 3] >= 0, ok), f"{where}: legal / illegal mask"
            assert np.array_equal(calls[~ok, 3], want[~ok, 3]), f"{where}: failure codes"
            assert np.array_equal(calls[:, 4], want[:, 4]), f"{where}: lengths"
            assert (d <= COST_RTOL).all(), f"{where}: costs"
            assert (r.xv, r.yv, r.thetav) == tuple(cyc.winner_vel), (where, (r.xv, r.yv, r.thetav), tuple(cyc.winner_vel))
            assert r.best_sample == cyc.best_call and r.n_points == cyc.n_points, (where, r.best_sample, cyc.best_call, r.n_points, cyc.n_points)
            assert _same_cost(r.cost, cyc.cost), (where, r.cost, cyc.cost)
            assert list(r.drive)[:2] == list(cyc.drive)[:2] and abs(r.drive[2] - cyc.drive[2]) <= DRIVE_YAW_BOUND, (where, list(r.drive), cyc.drive)
            t = fl.tp_trajectory(robot)
            assert t.shape == cyc.traj.shape and np.allclose(t, cyc.traj, rtol=0, atol=POINT_ATOL), f"{where}: trajectory points"
            st = fl.tp_state(robot, 1)[0]
            assert (st.flags, st.prev_x, st.prev_y, st.escape_x, st.escape_y, st.escape_theta) == (cyc.flags, *cyc.state), (where, st.flags, cyc.flags)
            for s, (want_cost, want_ok) in zip(cyc.post_samples, cyc.post):  # scoreTrajectory / checkTrajectory against this cycle's grids
                got = fl.tp_score_trajectory(robot, pos64, vel64, s)
                assert _same_cost(got, want_cost) and (got >= 0) == bool(want_ok), (where, tuple(s), got, want_cost)
    finally:
        fl.close()


@pytest.mark.parametrize("name", META["cases"])
def test_fleet_of_one(nav, name):
    _run(nav, name, 1, 0)


@pytest.mark.parametrize("name", META["cases"])
def test_robot_1_of_three(nav, name):
    _run(nav, name, 3, 1)


@pytest.mark.parametrize("name", META["cases"])
def test_other_allow_unknown(nav, name):
    assert META["allow_unknown_both_values_agree"] == len(META["cases"])
    _run(nav, name, 1, 0, other_allow_unknown=True)
