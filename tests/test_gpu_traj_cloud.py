"""navgpu_planner_set_trajectory_cloud / navgpu_planner_trajectory_cloud / navgpu_planner_sample_terms on the device against
the CPU oracle's record of the reference flow (tests/traj_cloud_ref.py; the model itself is pinned by tests/test_traj_cloud_model.py).

Fleets of 3 robots on 160 x 160 maps, 16 x 8 x 10 velocity samples (1584 - 1683 slots: several passes of the scan workgroup),
max_sim_steps 64; robots 0 and 2 are enabled, robot 1 is not.  Costs are compared for EQUALITY: both sides form the same fp64 sums in
the same order from integer-valued terms and the same scales, and exact ties between a partial sum and the incumbent are common - a sum
that is off in its last bit flips early-out decisions."""
import ctypes as C

import numpy as np
import pytest

import traj_cloud_ref as R

pytestmark = pytest.mark.gpu

ENABLED = (0, 2)
# (configuration, the three robots' scenes, oscillation flags set on both sides before the first cycle)
CASES = {
    "by_time": (R.config_kw(True), ("band", "open", "posts"), None),
    "by_distance": (R.config_kw(False), ("band", "open", "posts"), None),
    "sum_scores": (R.config_kw(True, sum_scores=1, occdist_scale=0.02), ("open", "band", "near_goal"), None),
    "by_distance_near_goal": (R.config_kw(False), ("open", "posts", "near_goal"), None),
    "oscillation_flags": (R.config_kw(True), ("open", "posts", "band"), R.OSC_FORWARD_POS_ONLY),
    "continued_acceleration": (R.config_kw(False, use_dwa=0), ("posts", "open", "band"), None),
}
# navgpu_dwa_config::rollout_trig = 1 is not among them: there the device takes cosf / sinf as its double functions rounded to float,
# which is within one unit in the last place of the host libm's float functions but not always equal to them
# (tests/test_gpu_parity_r4.py::test_device_float_trig_against_host_libm), so bit equality with the oracle's points is not the
# contract of that mode; test_float_trig_cloud_is_the_devices_own_rollout checks it against the device's own winner trajectory.


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _fleet(nav, cfg_kw, scenes, enabled=ENABLED, flags=None):
    from navigation_amd import _lib as N
    fl = nav.Fleet(len(scenes), R.N_CELLS, R.N_CELLS, R.RES, layers=N.LAYER_OBSTACLE, max_sim_steps=R.MAX_SIM_STEPS, max_plan=256,
                   keep_sample_costs=True)
    fl.configure_planner(nav.DwaConfig(**cfg_kw))
    fl.set_footprint(R.FOOTPRINT)
    fl.upload(N.GRID_MASTER, np.stack([s["master"] for s in scenes]))
    fl.set_plan()
    if flags is not None:
        fl.set_oscillation(np.full(len(scenes), flags, np.uint32), np.zeros((len(scenes), 3), np.float32))
    for i in enabled:
        fl.set_trajectory_cloud(True, first=i, count=1)
    return fl


def _cycle(fl, scenes):
    return fl.find_best_path(np.stack([s["pos"] for s in scenes]), np.stack([s["vel"] for s in scenes]), [s["plan"] for s in scenes])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(fl, orc, robot, cyc, tag):
    """one enabled robot's cloud and terms after a cycle against the oracle's record of the same cycle"""
    status, cref, cfull = cyc["status"], cyc["cref"], cyc["cfull"]
    scored = status == 1
    terms = fl.sample_terms(robot)
    assert len(terms) == len(status), tag
    assert np.array_equal(terms["status"], status), tag
    # the figures first: the largest difference of a cost from the oracle's, over the scored slots
    d_full = np.abs(terms["cost_full"][scored] - cfull[scored]).max(initial=0.0)
    d_ref = np.abs(terms["cost_ref"][scored] - cref[scored]).max(initial=0.0)
    print(f"{tag}: slots {len(status)} scored {int(scored.sum())} partial {int((scored & (cref != cfull)).sum())} "
          f"max|cost_full - oracle| {d_full:.3e} max|cost_ref - oracle| {d_ref:.3e}")
    assert np.array_equal(terms["cost_full"][scored], cfull[scored]), tag
    assert np.array_equal(terms["cost_ref"][scored], cref[scored]), tag
    for costs, mode in ((cref, True), (cfull, False)):
        want, member, n_points, offset = R.expected_cloud(orc, cyc, costs)
        got = fl.trajectory_cloud(robot, reference_costs=mode)
        assert got.shape == want.shape, (tag, mode, got.shape, want.shape)
        assert np.array_equal(_bits(got[:, [0, 1, 3]]), _bits(want[:, [0, 1, 3]])), (tag, mode)  # x, y, path_cost = theta: float bits
        assert not got[:, [2, 4, 5]].any(), (tag, mode)                                             # z, goal_cost, occ_cost
        assert np.array_equal(_bits(got[:, 6]), _bits(want[:, 6])), (tag, mode)                     # total_cost == float32(cost)
        if mode:
            assert np.array_equal(terms["member"] != 0, member), tag
            assert np.array_equal(terms["n_points"][scored], n_points[scored]) and not terms["n_points"][~scored].any(), tag
            assert np.array_equal(terms["point_offset"].astype(np.int64), offset), tag
    # the breakdown is consistent with itself: the rule, replayed on the device's own terms, gives the device's costs
    cfg = cyc["cfg"]
    sp, sg = R.RES * cfg.path_distance_bias * 0.5, R.RES * cfg.goal_distance_bias * 0.5
    gx, gy = cyc["plan_end"]
    far = (float(cyc["pos"][0]) - gx) ** 2 + (float(cyc["pos"][1]) - gy) ** 2 > cfg.forward_point_distance ** 2 * cfg.cheat_factor
    scales = [R.RES * cfg.occdist_scale, sg, sp if far else 0.0, sp, sg]
    best = R.incumbents(terms["cost_full"], terms["status"])
    for i in np.nonzero(scored)[0]:
        t = terms[i]
        assert R.replay_cost_ref(np.nan_to_num(t["critic"], nan=0.0), t["first_fail"], scales, best[i]) == t["cost_ref"], (tag, i)
        seen = [(scales[k] != 0 and k + 1 <= t["first_fail"]) for k in range(5)]
        assert np.array_equal(~np.isnan(t["critic"]), seen), (tag, i)
    return terms


@pytest.mark.parametrize("case", list(CASES))
def test_cloud_equals_the_reference_flow(nav, orc, case):
    cfg_kw, scene_names, flags = CASES[case]
    scenes = [R.scene(s) for s in scene_names]
    planners = [R.oracle_planner(orc, s, cfg_kw) for s in scenes]
    if flags is not None:
        for p in planners:
            p.set_oscillation(flags, (0, 0, 0))
    run = dict(planners=planners, flags=flags)
    fl = _fleet(nav, cfg_kw, scenes, flags=flags)
    try:
        for k in range(2):  # the second cycle is scored under the oscillation flags the first produced
            res = _cycle(fl, scenes)
            for robot in range(3):
                p = run["planners"][robot]
                flags_before = p.oscillation()[0]
                cyc = R.oracle_cycle(orc, p, scenes[robot])
                cyc["plan_end"] = scenes[robot]["plan"][-1]
                assert res[robot].best_index == cyc["result"].best_index and res[robot].n_valid == cyc["result"].n_valid, (case, k, robot)
                assert res[robot].oscillation_flags == p.oscillation()[0], (case, k, robot)
                if robot in ENABLED:
                    terms = _compare(fl, orc, robot, cyc, f"{case} cycle {k} robot {robot} flags {flags_before:#x}")
                    # the slots that fail the oscillation critic (-5): the backward samples under FORWARD_POS_ONLY
                    n5 = int(((cyc["status"] == 1) & (cyc["cfull"] == -5.0)).sum())
                    assert int((terms["first_fail"] == 0).sum()) == n5 and np.all(terms["cost_ref"][terms["first_fail"] == 0] == -5.0)
                    if run["flags"] is not None and k == 0 and scene_names[robot] == "open":
                        assert (flags_before & R.OSC_FORWARD_POS_ONLY) and n5 > 0
    finally:
        fl.close()


def _winner_points_equal_k_select(fl, robot, terms, cloud, res):
    """the points of the winning slot in the cloud are k_select's trajectory of the same cycle, narrowed to float: one step, two kernels"""
    w = res[robot].best_index
    assert w >= 0 and terms["member"][w]
    traj = fl.trajectory(robot)
    lo = int(terms["point_offset"][w])
    got = cloud[lo:lo + int(terms["n_points"][w])]
    assert len(traj) == len(got) == res[robot].n_points
    assert np.array_equal(_bits(got[:, [0, 1, 3]]), _bits(traj.astype(np.float32)))
    assert np.all(got[:, 6] == np.float32(res[robot].cost))


@pytest.mark.parametrize("case", ["by_time", "continued_acceleration"])
def test_winner_points_are_k_selects(nav, case):
    cfg_kw, scene_names, _ = CASES[case]
    scenes = [R.scene(s) for s in scene_names]
    fl = _fleet(nav, cfg_kw, scenes)
    try:
        res = _cycle(fl, scenes)
        for robot in ENABLED:
            _winner_points_equal_k_select(fl, robot, fl.sample_terms(robot), fl.trajectory_cloud(robot), res)
    finally:
        fl.close()


def test_float_trig_cloud_is_the_devices_own_rollout(nav, orc):
    """rollout_trig = 1 with continued acceleration.  Against the oracle (host cosf / sinf): the slots' point counts, which depend on
    the samples alone, and theta, which takes no trigonometry, are equal; x and y are within 64 x 2^-21 m - a float sine or cosine that
    differs by its last place moves a step's sum by at most |v| dt 2^-24 < 4e-9 m, which can turn the rounding of the new coordinate
    by one unit in its last place (2^-21 m for coordinates in [4, 8) m), once per step, over at most max_sim_steps = 64 steps.
    Against the device itself: membership, offsets and costs follow from its own terms by the rule, and the winner's points are
    k_select's."""
    cfg_kw = R.config_kw(False, use_dwa=0, rollout_trig=1)
    scene_names = ("posts", "open", "band")
    scenes = [R.scene(s) for s in scene_names]
    fl = _fleet(nav, cfg_kw, scenes)
    try:
        res = _cycle(fl, scenes)
        for robot in ENABLED:
            p = R.oracle_planner(orc, scenes[robot], cfg_kw)
            cyc = R.oracle_cycle(orc, p, scenes[robot])
            terms = fl.sample_terms(robot)
            scored = cyc["status"] == 1
            assert np.array_equal(terms["status"], cyc["status"])
            member = (terms["status"] == 1) & (terms["cost_ref"] >= 0)
            assert np.array_equal(terms["member"] != 0, member)
            assert np.array_equal(terms["point_offset"].astype(np.int64), np.concatenate([[0], np.cumsum(np.where(member, terms["n_points"], 0))[:-1]]))
            cloud = fl.trajectory_cloud(robot)
            assert len(cloud) == int(terms["n_points"][member].sum())
            assert np.array_equal(cloud[:, 6], np.repeat(terms["cost_ref"][member].astype(np.float32), terms["n_points"][member]))
            want, _, n_points, _ = R.expected_cloud(orc, cyc, np.where(member, 1.0, -1.0))  # the oracle's points of the device's members
            assert np.array_equal(terms["n_points"][scored], n_points[scored])
            assert want.shape == cloud.shape and np.array_equal(_bits(cloud[:, 3]), _bits(want[:, 3]))
            d = np.abs(cloud[:, :2].astype(np.float64) - want[:, :2]).max()
            print(f"float trig robot {robot}: {len(cloud)} points, max |x, y - oracle| {d:.3e} m, differing {int((cloud[:, :2] != want[:, :2]).any(axis=1).sum())}")
            assert d <= 64 * 2.0 ** -21
            _winner_points_equal_k_select(fl, robot, terms, cloud, res)
    finally:
        fl.close()


def test_capacity_and_determinism(nav):
    cfg_kw, scene_names, _ = CASES["by_distance"]
    scenes = [R.scene(s) for s in scene_names]
    fl = _fleet(nav, cfg_kw, scenes)
    try:
        _cycle(fl, scenes)
        L = fl.L
        for ref in (1, 0):
            n = L.navgpu_planner_trajectory_cloud(fl.h, 0, ref, None, 0)  # count only
            assert n > 1000
            full = np.full((n + 8, 7), -77.0, np.float32)
            assert L.navgpu_planner_trajectory_cloud(fl.h, 0, ref, full.ctypes.data_as(C.c_void_p), n + 8) == n
            assert np.all(full[n:] == -77.0) and not np.any(full[:n, 6] == -77.0)  # nothing behind the last point
            half = np.full((n, 7), -77.0, np.float32)
            assert L.navgpu_planner_trajectory_cloud(fl.h, 0, ref, half.ctypes.data_as(C.c_void_p), n // 2) == n
            assert np.array_equal(_bits(half[:n // 2]), _bits(full[:n // 2])) and np.all(half[n // 2:] == -77.0)
            again = np.full((n + 8, 7), -77.0, np.float32)
            assert L.navgpu_planner_trajectory_cloud(fl.h, 0, ref, again.ctypes.data_as(C.c_void_p), n + 8) == n
            assert again.tobytes() == full.tobytes()
        assert fl.sample_terms(0).tobytes() == fl.sample_terms(0).tobytes()
        # a capacity with no buffer is an argument error
        assert L.navgpu_planner_trajectory_cloud(fl.h, 0, 1, None, 4) == -1
        assert L.navgpu_planner_trajectory_cloud(fl.h, 3, 1, None, 0) == -1
    finally:
        fl.close()


def _observable(fl, n):
    res = fl.results()
    flags, prev = fl.oscillation()
    return ([bytes(r) for r in res], [tuple(a.tobytes() for a in fl.samples(i)) for i in range(n)], flags.tobytes(), prev.tobytes(),
            [fl.trajectory(i).tobytes() for i in range(n)])


@pytest.mark.parametrize("case", ["by_time", "by_distance"])
def test_nothing_changes_for_anyone(nav, case):
    """plan results (n_scored and n_valid included), sample costs and oscillation state of every robot - the enabled ones too - equal
    those of a fleet that enables nobody, over two cycles"""
    cfg_kw, scene_names, _ = CASES[case]
    scenes = [R.scene(s) for s in scene_names]
    plain, flagged = _fleet(nav, cfg_kw, scenes, enabled=()), _fleet(nav, cfg_kw, scenes)
    try:
        for k in range(2):
            _cycle(plain, scenes)
            _cycle(flagged, scenes)
            a, b = _observable(plain, 3), _observable(flagged, 3)
            assert a == b, (case, k)
            assert all(r.n_scored > 0 for r in flagged.results())
    finally:
        plain.close()
        flagged.close()


def test_states(nav):
    from navigation_amd import _lib as N
    ERR_INVALID, ERR_STATE = -1, -5
    cfg_kw, scene_names, _ = CASES["by_time"]
    scenes = [R.scene(s) for s in scene_names]
    fl = _fleet(nav, cfg_kw, scenes)
    try:
        L = fl.L
        st = (N.SampleTerms * 4)()
        # enabled, no cycle yet
        assert L.navgpu_planner_trajectory_cloud(fl.h, 0, 1, None, 0) == ERR_STATE
        assert L.navgpu_planner_sample_terms(fl.h, 0, C.cast(st, C.c_void_p), 4) == ERR_STATE
        _cycle(fl, scenes)
        assert L.navgpu_planner_trajectory_cloud(fl.h, 0, 1, None, 0) > 0
        assert L.navgpu_planner_sample_terms(fl.h, 2, C.cast(st, C.c_void_p), 4) >= 1584
        # robot 1 is not enabled
        assert L.navgpu_planner_trajectory_cloud(fl.h, 1, 1, None, 0) == ERR_STATE
        assert L.navgpu_planner_sample_terms(fl.h, 1, None, 0) == ERR_STATE
        # staged again after the cycle
        fl.stage_poses(scenes[0]["pos"][None], scenes[0]["vel"][None], first=0)
        assert L.navgpu_planner_trajectory_cloud(fl.h, 0, 1, None, 0) == ERR_STATE
        assert L.navgpu_planner_trajectory_cloud(fl.h, 2, 1, None, 0) > 0  # (robot 2 was not)
        fl.planner_cycle()
        assert L.navgpu_planner_trajectory_cloud(fl.h, 0, 1, None, 0) > 0
        # reconfigured after the cycle
        fl.configure_planner(nav.DwaConfig(**cfg_kw))
        assert L.navgpu_planner_trajectory_cloud(fl.h, 2, 1, None, 0) == ERR_STATE
        # disabled again: as for a robot that never was
        fl.set_trajectory_cloud(False, first=0, count=1)
        fl.planner_cycle()
        assert L.navgpu_planner_trajectory_cloud(fl.h, 0, 1, None, 0) == ERR_STATE
        assert L.navgpu_planner_trajectory_cloud(fl.h, 2, 1, None, 0) > 0
        # two cycles in flight
        assert L.navgpu_planner_set_cycles_in_flight(fl.h, 2) == ERR_STATE
        fl.set_trajectory_cloud(False)
        fl.set_cycles_in_flight(2)
        assert L.navgpu_planner_set_trajectory_cloud(fl.h, 0, 1, 1) == ERR_STATE
        fl.set_cycles_in_flight(1)
    finally:
        fl.close()
    # a 17th enabled robot
    big = nav.Fleet(18, 32, 32, R.RES, layers=N.LAYER_OBSTACLE, max_sim_steps=R.MAX_SIM_STEPS)
    try:
        assert N.TRAJ_CLOUD_MAX_ROBOTS == 16
        assert big.L.navgpu_planner_set_trajectory_cloud(big.h, 0, 17, 1) == ERR_INVALID  # all or nothing
        big.set_trajectory_cloud(True, first=0, count=16)
        big.set_trajectory_cloud(True, first=3, count=2)  # already enabled: no new robot
        assert big.L.navgpu_planner_set_trajectory_cloud(big.h, 16, 1, 1) == ERR_INVALID
        big.set_trajectory_cloud(False, first=5, count=1)
        big.set_trajectory_cloud(True, first=17, count=1)
        assert big.L.navgpu_planner_set_trajectory_cloud(big.h, 5, 1, 1) == ERR_INVALID
    finally:
        big.close()
