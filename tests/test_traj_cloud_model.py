"""The model behind navgpu_planner_trajectory_cloud, on the CPU oracle alone, for the inputs tests/test_gpu_traj_cloud.py uses.

SimpleScoredSamplingPlanner::scoreTrajectory (simple_scored_sampling_planner.cpp:50-79) stops summing once a sample is worse than
the incumbent, so all_explored[i].cost_ - the cost DWAPlanner's trajectory cloud carries (dwa_planner.cpp:318-348) - is a partial
sum for most samples.  The device reproduces that flow from the full costs: the incumbent slot i sees is the exclusive prefix
minimum of the full costs of the valid slots before it.  Checked here slot by slot against the oracle's two records
(SampleRecord::cost_ref and cost_full), together with the counts that say the inputs reach the cases."""
import numpy as np
import pytest

import traj_cloud_ref as R

CASES = [("band", True, {}), ("band", False, {}), ("posts", True, {}), ("posts", False, {}), ("open", True, dict(sum_scores=1, occdist_scale=0.02)),
         ("open", False, {}), ("near_goal", True, {})]


def _cycles(orc, name, by_time, kw, n=2, flags=None):
    sc = R.scene(name)
    p = R.oracle_planner(orc, sc, R.config_kw(by_time, **kw))
    if flags is not None:
        p.set_oscillation(flags, (0, 0, 0))
    return [R.oracle_cycle(orc, p, sc) for _ in range(n)]


def _check_prefix_minimum(cyc):
    cref, cfull, status = cyc["cref"], cyc["cfull"], cyc["status"]
    best = R.incumbents(cfull, status)
    for i in np.nonzero(status == 1)[0]:
        if cref[i] == cfull[i]:
            continue
        if cfull[i] >= 0:
            assert best[i] > 0 and best[i] < cref[i] <= cfull[i], (i, best[i], cref[i], cfull[i])
        else:
            assert best[i] > 0 and cref[i] > best[i], (i, best[i], cref[i], cfull[i])
    # a slot that was cut short never becomes the incumbent: the winner is the first minimum of the full costs
    valid = (status == 1) & (cfull >= 0)
    if valid.any():
        assert cyc["result"].best_index == int(np.nonzero(valid & (cfull == cfull[valid].min()))[0][0])
        assert cyc["result"].cost == cfull[valid].min()


@pytest.mark.parametrize("name,by_time,kw", CASES)
def test_incumbent_is_the_prefix_minimum_of_the_full_costs(orc, name, by_time, kw):
    for cyc in _cycles(orc, name, by_time, kw):
        assert 1584 <= len(cyc["status"]) <= 1683
        _check_prefix_minimum(cyc)


def test_inputs_reach_the_cases(orc):
    partial = ref_only = 0
    codes, rejected = set(), 0
    for name, by_time, kw in CASES:
        cyc = _cycles(orc, name, by_time, kw, n=1)[0]
        s = cyc["status"] == 1
        partial += int((s & (cyc["cref"] != cyc["cfull"])).sum())
        ref_only += int((s & (cyc["cref"] >= 0) & (cyc["cfull"] < 0)).sum())
        codes |= set(cyc["cfull"][s & (cyc["cfull"] < 0)].tolist())
        rejected += int((~s).sum())
        if name == "band":  # the robot that faces away from its plan: nearly every scored slot is cut short, hundreds before the critic that fails
            assert int((s & (cyc["cref"] != cyc["cfull"])).sum()) >= 500 and int((s & (cyc["cref"] >= 0) & (cyc["cfull"] < 0)).sum()) >= 300
        if not by_time:  # variable point counts
            n = np.array([R.orc_points(orc, cyc, i) for i in np.nonzero(s)[0][::37]])
            assert n.min() < n.max()
    assert partial >= 500 and ref_only >= 300, (partial, ref_only)
    assert -6.0 in codes and -3.0 in codes, codes
    assert rejected > 0


def test_oscillation_flags_fail_backward_samples(orc):
    cyc = _cycles(orc, "open", True, {}, n=1, flags=R.OSC_FORWARD_POS_ONLY)[0]
    s = cyc["status"] == 1
    assert int((s & (cyc["cfull"] == -5.0)).sum()) > 0
    assert np.array_equal(cyc["cref"][s & (cyc["cfull"] == -5.0)], cyc["cfull"][s & (cyc["cfull"] == -5.0)])  # the first critic: never cut short
    _check_prefix_minimum(cyc)


def test_near_goal_switches_alignment_off(orc):
    sc = R.scene("near_goal")
    cfg = R.config_kw(True)
    gx, gy = sc["plan"][-1]
    d2 = (float(sc["pos"][0]) - gx) ** 2 + (float(sc["pos"][1]) - gy) ** 2
    assert d2 <= 0.325 ** 2  # forward_point_distance^2 * cheat_factor (dwa_planner.cpp:279-285), the defaults
    assert "forward_point_distance" not in cfg and "cheat_factor" not in cfg


def test_expected_cloud_helper(orc):
    """the helper's own bookkeeping: offsets are the running point count of the members, and the two modes differ as the issue says"""
    cyc = _cycles(orc, "band", False, {}, n=1)[0]
    pts, member, n_points, offset = R.expected_cloud(orc, cyc, cyc["cref"])
    assert len(pts) == int(n_points[member].sum()) and np.array_equal(offset, np.concatenate([[0], np.cumsum(np.where(member, n_points, 0))[:-1]]))
    assert np.all(pts[:, 2] == 0) and np.all(pts[:, 4] == 0) and np.all(pts[:, 5] == 0)
    full_pts, full_member, _, _ = R.expected_cloud(orc, cyc, cyc["cfull"])
    assert full_member.sum() < member.sum() and np.all(member[full_member])
    assert n_points[cyc["status"] == 1].min() >= 1 and n_points.max() <= R.MAX_SIM_STEPS
