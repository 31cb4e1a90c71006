"""navgpu_move_base_plan_service on the GPU: MoveBase::planService's goal search as batches of candidate plans, against the yardstick's
loop (tests/move_base_ref.py: one makePlan after the other, stopping at the first success) driven by the library's own single-plan
make_plan on a handle of one plan.

Scene: a 64 x 64 map at 0.05 m with a lethal block of 11 x 11 cells; the first request's goal is the block's middle.  The search
increment is 3 cells, so the exact goal and the whole first ring (offsets of 3 cells) lie in the block and ring 2 (6 cells) outside
it: the winner is the first candidate of ring 2, candidate 1 + 8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import move_base_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
N_CELLS, RES = 64, 0.05
FRAME = (0.0, 0.0, RES)
START = (0.525, 0.525, 0.3)
BLOCKED = (32.5 * RES, 32.5 * RES, 1.1)  # the middle of the block
REQUESTS = [dict(start=START, goal=BLOCKED, frame=FRAME, tolerance=0.5),                 # 49 candidates, the winner in ring 2
            dict(start=START, goal=(2.625, 0.625, -0.4), frame=FRAME, tolerance=0.5),    # the exact goal is free: winner 0
            dict(start=START, goal=BLOCKED, frame=FRAME, tolerance=0.2)]                 # one ring, all of it in the block: no winner


def _map():
    m = np.zeros((N_CELLS, N_CELLS), np.uint8)
    m[27:38, 27:38] = 254
    return m


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    return nav


@pytest.fixture(scope="module", params=["global_planner", "navfn_ros"])
def family(request):
    return request.param


def _make(nf, family, first, starts, goals):
    """the family's make_plan and plans read on slots first ..: -> list of (n, 3) arrays"""
    if family == "global_planner":
        res = nf.make_plan(FRAME, starts, goals, first=first, orientation_mode=1)
        poses, off = nf.plans(first=first, count=len(res))
    else:
        res = nf.navfn_ros_make_plan(FRAME, starts, goals, tolerances=0.0, first=first)
        poses, off = nf.navfn_ros_plans(first=first, count=len(res))
    return [poses[off[k]:off[k + 1]] for k in range(len(res))]


def _read(nf, family, slot):
    poses, off = nf.plans(first=slot, count=1) if family == "global_planner" else nf.navfn_ros_plans(first=slot, count=1)
    return poses[off[0]:off[1]]


@pytest.fixture(scope="module")
def expected(nav, family):
    """the yardstick's loop over single makePlan calls of the same build, per request: (winner, tried, plan); computed once"""
    one = nav.NavFn(N_CELLS, N_CELLS, 1)
    try:
        one.set_costmap(_map(), cost_mode=0 if family == "global_planner" else 1)
        out = []
        for rq in REQUESTS:
            out.append(R.plan_service(rq["goal"], RES, rq["tolerance"], lambda g: _make(one, family, 0, [rq["start"]], [g])[0]))
    finally:
        one.close()
    assert [(w, t) for w, t, _ in out] == [(9, 10), (0, 1), (-1, 9)], [(w, t) for w, t, _ in out]
    assert out[0][2][-1].tolist() == list(BLOCKED) and len(out[0][2]) > 10 and out[1][2][-1, 2] == -0.4
    return out


@pytest.mark.parametrize("slots", [49, 5])
def test_plan_service_matches_the_sequential_search(nav, family, expected, slots):
    from navigation_amd import _lib as N
    fam = N.PLAN_FAMILY_GLOBAL_PLANNER if family == "global_planner" else N.PLAN_FAMILY_NAVFN_ROS
    nf = nav.NavFn(N_CELLS, N_CELLS, 1 + 3 * slots)  # the requests' slots start at 1: first_slot is honoured
    try:
        nf.set_costmap(_map(), cost_mode=0 if family == "global_planner" else 1)
        res, won = nf.plan_service(fam, REQUESTS, slots, first_slot=1, orientation_mode=1)
        for q, (r, (winner, tried, plan)) in enumerate(zip(res, expected)):
            n_cand = len(R.plan_service_candidates(REQUESTS[q]["goal"][:2], RES, REQUESTS[q]["tolerance"]))
            assert (r.winner, r.tried, r.n_candidates, r.n_poses) == (winner, tried, n_cand, len(plan)), (q, r.winner, r.tried, r.n_poses)
            assert r.rounds == (-(-tried // slots) if winner >= 0 else -(-n_cand // slots)), (q, r.rounds)
            if winner < 0:
                assert r.slot == -1 and won[q].n_poses == 0
                continue
            assert r.slot == 1 + q * slots + winner % slots
            got = _read(nf, family, r.slot)
            assert got.tobytes() == plan.tobytes(), (q, len(got), len(plan))
            assert won[q].status == N.MAKE_PLAN_OK and won[q].n_poses == len(plan) - (1 if winner else 0)
        # a range read over a request's slots sees the appended pose in place too
        w = res[0]
        first = 1
        poses, off = nf.plans(first=first, count=slots) if family == "global_planner" else nf.navfn_ros_plans(first=first, count=slots)
        k = w.slot - first
        assert poses[off[k]:off[k + 1]].tobytes() == expected[0][2].tobytes()
    finally:
        nf.close()


def test_winner_is_handed_over_with_the_appended_goal(nav, family, expected):
    from navigation_amd import _lib as N, synth
    fam = N.PLAN_FAMILY_GLOBAL_PLANNER if family == "global_planner" else N.PLAN_FAMILY_NAVFN_ROS
    cfg = nav.DwaConfig(vx_samples=6, vy_samples=1, vth_samples=7, sim_time=1.0, sim_granularity=0.1, discretize_by_time=1)
    fl = nav.Fleet(2, N_CELLS, N_CELLS, RES, layers=N.LAYER_OBSTACLE, max_sim_steps=32, max_plan=256)
    nf = nav.NavFn(N_CELLS, N_CELLS, 49)
    try:
        fl.configure_planner(cfg)
        fl.set_footprint(synth.FOOTPRINT)
        fl.upload(N.GRID_MASTER, np.stack([np.zeros((N_CELLS, N_CELLS), np.uint8), _map()]))
        fl.configure_local_planner(xy_goal_tolerance=0.15, yaw_goal_tolerance=0.08, rot_stopped_vel=0.01, trans_stopped_vel=0.01,
                                   max_rot_vel=cfg.max_rot_vel, min_rot_vel=cfg.min_rot_vel, acc_lim_x=cfg.acc_lim_x, acc_lim_y=cfg.acc_lim_y,
                                   acc_lim_theta=cfg.acc_lim_theta, sim_period=cfg.sim_period, prune_plan=1, latch_xy_goal_tolerance=0)
        fl.reserve_global_plans(512)
        mode = 0 if family == "global_planner" else 1
        # the slots' costs come from ONE fleet instance, the second one: the same bytes as the host map gives
        nf.set_costmap_from_fleet_instance(fl, 1, cost_mode=mode)
        from_fleet = [nf.costarr(k) for k in (0, 17, 48)]
        nf.set_costmap(_map(), cost_mode=mode)
        assert all(np.array_equal(a, nf.costarr(k)) for a, k in zip(from_fleet, (0, 17, 48)))
        nf.set_costmap_from_fleet_instance(fl, 1, cost_mode=mode)
        res, _ = nf.plan_service(fam, REQUESTS[:1], 49, orientation_mode=1)
        assert res[0].winner == 9 and res[0].rounds == 1
        rec = fl.handover_global_plans(nf, fam, [START[:2]], 0, count=1, first=1, nav_first=res[0].slot)
        assert (rec[0].decision, rec[0].new_len) == (N.HANDOVER_ADOPT, len(expected[0][2]))
        assert fl.global_plan(1).tobytes() == expected[0][2].tobytes()
        assert fl.global_plan(1)[-1].tolist() == list(BLOCKED)
    finally:
        nf.close()
        fl.close()


def test_too_many_candidates_is_refused_before_anything_runs(nav, family):
    from navigation_amd import _lib as N
    from navigation_amd._lib import NavgpuError
    fam = N.PLAN_FAMILY_GLOBAL_PLANNER if family == "global_planner" else N.PLAN_FAMILY_NAVFN_ROS
    nf = nav.NavFn(N_CELLS, N_CELLS, 4)
    try:
        nf.set_costmap(_map(), cost_mode=0 if family == "global_planner" else 1)
        many = dict(start=START, goal=BLOCKED, frame=(0.0, 0.0, 0.001), tolerance=1.0)
        with pytest.raises(NavgpuError):
            nf.plan_service(fam, [REQUESTS[1], many], 2)
        with pytest.raises(NavgpuError):  # nothing has run: no plan was made on any slot
            _read(nf, family, 0)
        with pytest.raises(NavgpuError):  # the slots do not fit the handle
            nf.plan_service(fam, REQUESTS[:1], 5)
    finally:
        nf.close()
