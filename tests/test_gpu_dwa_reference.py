"""The DWA scoring kernels (k_samples, k_score_sweep, k_score_gen*, k_score_explicit*, k_score_terms*, k_select) and the MapGrid
wavefronts against the reference's own numbers: tests/golden/g15_dwa_reference.npz, written by tools/make_dwa_goldens.py from
dwa_local_planner::DWAPlanner and the base_local_planner classes compiled in place.  Reads the fixture only: no reference tree, no
CPU oracle.  Need a real MI355X.

Bar (that of tests/test_gpu_parity.py::_check_planner): grids, sample velocities, accept mask, valid / invalid mask, failure codes,
best_index, n_scored, n_valid, oscillation flags and winner velocities bit-equal; costs within 1e-5; trajectory points within 1e-6.
The terms pass stores doubles: its raw critic values (cell counts, costmap bytes, their sums and products) are held to rtol 1e-9,
five orders below what one cell changes (1 / 25601) and five above what 150 double operations can lose (2e-14)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwa_reference_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

G, META = D.load()
COST_ATOL, POINT_ATOL = 1e-5, 1e-6


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _expected_terms(cyc):
    """What navgpu_sample_terms holds per slot by its contract (include/navgpu.h), from the reference's raw critic values: the five
    critics after the oscillation one, NaN where scoreTrajectory never evaluated the critic (scale 0, or behind the first failure)."""
    want = np.full((cyc.n_slots, 5), np.nan)
    first_fail = np.full(cyc.n_slots, 6, np.int32)
    for s in np.nonzero(cyc.accepted)[0]:
        for i in range(6):
            if cyc.scale[i] == 0.0:
                continue
            if i:
                want[s, i - 1] = cyc.critic[s, i]
            if cyc.critic[s, i] < 0:
                first_fail[s] = i
                break
    return want, first_fail


def _run(nav, name, n_inst, robot):
    from navigation_amd import _lib as N
    c, costmap, cycles, check_ok = D.case(G, META, name)
    cfg = dict(c["cfg"], rollout_trig=META["rollout_trig"])
    maps = [costmap] * n_inst
    if n_inst > 1:  # the other robots carry other maps of the same size: batch indexing
        maps = [np.ascontiguousarray(costmap[::-1]), costmap, np.ascontiguousarray(costmap.T)]
        assert not np.array_equal(maps[0], costmap) and not np.array_equal(maps[2], costmap)
    fl = nav.Fleet(n_inst, c["size_x"], c["size_y"], c["res"], layers=N.LAYER_OBSTACLE, keep_sample_costs=True,
                   max_sim_steps=c["max_sim_steps"], max_plan=256)
    try:
        fl.configure_planner(nav.DwaConfig(**cfg))
        fl.set_footprint(c["fp"])
        fl.upload(N.GRID_MASTER, np.stack(maps))
        for m, a, y in zip(D.MAP_GRID_CRITICS, c["agg"], c["yshift"]):
            if a or y:
                fl.set_map_grid_options(m, D.AGGREGATIONS[a], y)
        fl.set_trajectory_cloud(True, first=robot, count=1)
        for k, cyc in enumerate(cycles):
            where = f"{name} cycle {k} robot {robot} of {n_inst}"
            if cyc.set_plan:
                fl.set_plan()
            r = fl.find_best_path(np.stack([cyc.pos] * n_inst), np.stack([cyc.vel] * n_inst), [cyc.plan] * n_inst)[robot]
            for gid, which in ((N.GRID_PATH, 0), (N.GRID_GOAL, 1), (N.GRID_GOAL_FRONT, 2)):
                got = fl.download(gid, robot, 1)[0]
                assert np.array_equal(got.astype(np.float64), cyc.grid[which].astype(np.float64)), f"{where}: MapGrid {which}"
            cost, status, vels = fl.samples(robot)
            acc = cyc.accepted
            full = cyc.total_full[acc]
            assert len(cost) == cyc.n_slots == r.n_samples, where
            assert np.array_equal(vels.view(np.uint32), cyc.samples.view(np.uint32)), f"{where}: sample velocities"
            assert np.array_equal(status == 1, acc), f"{where}: accept mask"
            got = cost[acc]
            d = np.abs(got[full >= 0] - full[full >= 0]).max(initial=0.0) if np.array_equal(got < 0, full < 0) else float("nan")
            print(f"{where}: slots {cyc.n_slots} scored {int(acc.sum())} valid {int((full >= 0).sum())} max|cost - reference| {d:.3e}")
            assert np.array_equal(got < 0, full < 0), f"{where}: valid / invalid mask"
            assert np.array_equal(got[full < 0], full[full < 0]), f"{where}: failure codes"
            assert np.allclose(got[full >= 0], full[full >= 0], rtol=0, atol=COST_ATOL), f"{where}: costs"
            assert r.best_index == cyc.best_index, (where, r.best_index, cyc.best_index)
            assert r.n_scored == int(acc.sum()) and r.n_valid == int((full >= 0).sum()), where
            assert r.oscillation_flags == cyc.flags, (where, r.oscillation_flags, cyc.flags)
            flags, prev = fl.oscillation(robot, 1)
            assert flags[0] == cyc.flags and np.array_equal(prev[0], cyc.prev), f"{where}: oscillation state"
            if cyc.found:
                assert abs(r.cost - cyc.cost) <= COST_ATOL, where
                assert (r.xv, r.yv, r.thetav) == tuple(np.float32(v) for v in cyc.winner_vel), f"{where}: winner velocities"
                assert list(r.drive) == [float(v) for v in cyc.winner_vel], where
                t = fl.trajectory(robot)
                assert t.shape == cyc.traj.shape and np.allclose(t, cyc.traj, rtol=0, atol=POINT_ATOL), f"{where}: trajectory points"
            else:
                assert r.cost < 0 and list(r.drive) == [0.0, 0.0, 0.0], where
            # the terms pass behind the trajectory cloud
            terms = fl.sample_terms(robot)
            want, first_fail = _expected_terms(cyc)
            assert len(terms) == cyc.n_slots and np.array_equal(terms["status"] == 1, acc), f"{where}: terms status"
            assert np.array_equal(terms["n_points"][acc], cyc.slot_points[acc]) and not terms["n_points"][~acc].any(), f"{where}: step counts"
            assert np.array_equal(terms["first_fail"][acc], first_fail[acc]), f"{where}: first failing critic"
            assert np.array_equal(np.isnan(terms["critic"][acc]), np.isnan(want[acc])), f"{where}: critics evaluated"
            seen = ~np.isnan(want[acc])
            assert np.allclose(terms["critic"][acc][seen], want[acc][seen], rtol=1e-9, atol=COST_ATOL), f"{where}: raw critic values"
            for field, ref in (("cost_full", cyc.total_full), ("cost_ref", cyc.total_ref)):
                tv, rv = terms[field][acc], ref[acc]
                assert np.array_equal(tv < 0, rv < 0) and np.array_equal(tv[rv < 0], rv[rv < 0]), f"{where}: terms {field} codes"
                assert np.allclose(tv[rv >= 0], rv[rv >= 0], rtol=1e-9, atol=COST_ATOL), f"{where}: terms {field}"
            assert (terms["cost_full"][~acc] == -1.0).all(), where
        for sample, ok in zip(c["checks"], check_ok):  # DWAPlanner::checkTrajectory with the last cycle's pose and velocity
            assert fl.check_trajectory(robot, sample) == bool(ok), f"{name} robot {robot} of {n_inst}: checkTrajectory{tuple(sample)}"
    finally:
        fl.close()


@pytest.mark.parametrize("name", META["cases"])
def test_fleet_of_one(nav, name):
    _run(nav, name, 1, 0)


@pytest.mark.parametrize("name", META["cases"])
def test_robot_1_of_three(nav, name):
    _run(nav, name, 3, 1)
