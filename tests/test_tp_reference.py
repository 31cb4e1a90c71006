"""CPU checks of the legacy TrajectoryPlanner yardstick: tests/golden/g16_tp_reference.npz is what the reference's own
base_local_planner::TrajectoryPlanner computes (compiled in place by tools/make_tp_goldens.py), the fixture reaches the branches of
createTrajectories and generateTrajectory, and oracle/trajectory_planner_oracle.hpp - what the GPU tests of k_tp_within, k_tp_rollout
and the host replay compare with - reproduces it bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tp_reference_cases as T  # noqa: E402
import make_tp_goldens as M  # noqa: E402
from test_dwa_reference import DRIVE_YAW_BOUND  # noqa: E402

needs_reference = pytest.mark.skipif(not M.available(), reason="the reference base_local_planner / costmap_2d trees are not on this machine")


@pytest.fixture(scope="module")
def golden():
    return T.load()


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path):
    out = tmp_path / "g16.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_tp_goldens.py"), "--out", str(out)], check=True, capture_output=True)
    new, old = np.load(out), np.load(T.GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = old[k], new[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), k
        else:
            assert np.array_equal(a, b), k
    golden_dir = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(T.GOLDEN) <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if not f.startswith("g16_"))


def _in_lethal(c, costmap, x, y):
    mx, my = int((x - c["origin"][0]) / c["res"]), int((y - c["origin"][1]) / c["res"])
    return costmap[my, mx] == T.LETHAL


def _on_map(c, x, y):
    return c["origin"][0] <= x < c["origin"][0] + c["size_x"] * c["res"] and c["origin"][1] <= y < c["origin"][1] + c["size_y"] * c["res"]


def test_golden_cases_cover_the_branches(golden):
    """From the recorded data alone.  What createTrajectories cannot reach is said here and not pretended:
      * the first flag-update block (:704-725) is entered with a winner of the forward grid, the holonomic pair or the in-place stage;
        with xv_ <= 0 that is a sample with vy = 0 (the pair has xv_ = 0.1), so its two strafing branches never run;
      * the second block (:802-822) is entered only when those stages left nothing legal, with a winner of the y_vels stage
        (thetav_ = 0), so its two rotating branches never run.  strafe_left / strafe_right and the stuck_*_strafe flags therefore come
        from the second block alone, rotating_* and stuck_left / stuck_right from the first;
      * the unclamped in-place loop variable is not a recorded quantity; that the `vtheta_samp > dvtheta` gate rejects a legal call shows
        where dvtheta is x / 0 or 0 / 0 (vtheta_samples = 1: the gate rejects every call) - see below;
      * `impossible_cost <= path_dist` (:335) cannot be the only true half of the -2 test on a map without unknown cells: the local goal
        that seeds goal_map_ is the last of the poses that seed path_map_ (map_grid.cpp:189-202, :225-238), both wavefronts apply one
        obstacle rule (:110-116) and within_robot only opens cells to path_map_, so every cell goal_map_ reaches, path_map_ reaches;
      * -1 by leaving the map: with a polygon footprint a vertex leaves before the centre does, and CostmapModel answers -1 for it
        before the worldToMap test of generateTrajectory (:272) can fail (`border`).  With fewer than three vertices CostmapModel looks
        at the centre only, and :272 is what fails first (`fp2_off_border`)."""
    g, meta = golden
    cases = {n: T.case(g, meta, n) for n in meta["cases"]}
    every = [(n, c, m, k, cy) for n, (c, m, cycles) in cases.items() for k, cy in enumerate(cycles)]
    # ---- the fixture's frame: sizes, one non-square map, one negative origin, no unknown cells, both allow_unknown values (inert)
    shapes = {m.shape for _, m, _ in cases.values()}
    assert all(64 <= min(s) and max(s) <= 160 for s in shapes) and any(s[0] != s[1] for s in shapes)
    assert any(c["origin"][0] < 0 and c["origin"][1] < 0 for c, _, _ in cases.values())
    assert not any((m == T.NOINFO).any() for _, m, _ in cases.values())
    assert {c["allow_unknown"] for c, _, _ in cases.values()} == {0, 1}
    assert meta["allow_unknown_both_values_agree"] == len(cases)  # the generator ran every case with both values and compared every double
    assert meta["knife_edge_min_cells"] >= meta["knife_edge_bound_cells"] == 1e-9
    assert max(len(cycles) for _, _, cycles in cases.values()) <= 14

    # ---- winners, by the stage of the winning call
    def winners(stage):
        return [(n, k, cy) for n, _, _, k, cy in every if cy.stage_of(cy.best_call) == stage]
    assert any(cy.winner_vel[0] > 0 and cy.cost >= 0 for _, _, cy in winners(T.FORWARD))
    assert {tuple(cy.winner_vel) for _, _, cy in winners(T.PAIR)} == {(0.1, 0.1, 0.0), (0.1, -0.1, 0.0)}
    assert {np.sign(cy.winner_vel[2]) for _, _, cy in winners(T.IN_PLACE)} == {-1.0, 1.0}
    assert all(cy.winner_vel[0] == 0.0 and cy.winner_vel[1] == 0.0 for _, _, cy in winners(T.IN_PLACE))
    assert {np.sign(cy.winner_vel[1]) for _, _, cy in winners(T.Y_VELS)} == {-1.0, 1.0}
    backing = winners(T.BACKUP)
    assert all(cy.best_call == len(cy.calls) - 1 and cy.winner_vel[0] == cy.cfg["backup_vel"] for _, _, cy in backing)
    patched = [cy for _, _, cy in backing if cy.calls[-1][3] == -1.0]
    assert patched and all(cy.cost == 1.0 and cy.drive[0] == cy.cfg["backup_vel"] for cy in patched)          # -1 patched to 1.0
    no_goal = [cy for _, _, cy in backing if cy.calls[-1][3] == -2.0]
    assert no_goal and all(cy.cost == -2.0 and not cy.flags & T.ESCAPING and not cy.drive.any() for cy in no_goal)  # -2: no escape mode
    legal = [cy for _, _, cy in backing if cy.calls[-1][3] >= 0]
    assert legal and all(cy.cost == cy.calls[-1][3] and cy.flags & T.ESCAPING for cy in legal)                # backing up legally
    # ---- escape mode: entered, a cycle that finds it set skips the forward stage and the pair, cleared by distance and by angle
    escaping = [(n, k, cy) for n, _, _, k, cy in every if cy.entry_flags & T.ESCAPING]
    assert escaping and all(not cy.stage_calls(T.FORWARD) and not cy.stage_calls(T.PAIR) for _, _, cy in escaping)
    assert all(len(cy.calls) < len(cases[n][2][0].calls) for n, _, cy in escaping)
    cleared = [(n, cy) for n, _, cy in escaping if not cy.flags & T.ESCAPING]
    by_distance = [n for n, cy in cleared if np.hypot(cy.pos[0] - cy.state[2], cy.pos[1] - cy.state[3]) > cy.cfg["escape_reset_dist"]]
    by_angle = [n for n, cy in cleared if np.hypot(cy.pos[0] - cy.state[2], cy.pos[1] - cy.state[3]) <= cy.cfg["escape_reset_dist"] and
                abs(float(cy.pos[2]) - cy.state[4]) > cy.cfg["escape_reset_theta"]]
    assert by_distance and by_angle and set(by_distance).isdisjoint(by_angle), (by_distance, by_angle)
    assert any(cy.stage_of(cy.best_call) == T.IN_PLACE for _, _, cy in escaping)  # turning in place while escaping
    # ---- flags: every bit seen set; a stuck flag standing at the entry of a cycle whose stage has legal calls; cleared by distance
    seen = 0
    for _, _, _, _, cy in every:
        seen |= cy.flags
    assert seen == (1 << 9) - 1, bin(seen)

    def stage_legal(cy, stage):
        return any(cy.calls[i][3] >= 0 for i in cy.stage_calls(stage))
    assert any(cy.entry_flags & (T.STUCK_LEFT | T.STUCK_RIGHT) and stage_legal(cy, T.IN_PLACE) for _, _, _, _, cy in every)
    for bit, blocked_sign in ((T.STUCK_LEFT_STRAFE, 1.0), (T.STUCK_RIGHT_STRAFE, -1.0)):
        # the gate decides: the cheapest legal y_vels call has the blocked sign, the winner has the other
        hit = [cy for _, _, _, _, cy in every if cy.entry_flags & bit and cy.stage_of(cy.best_call) == T.Y_VELS]
        assert any(np.sign(min((cy.calls[i][3], cy.calls[i][1]) for i in cy.stage_calls(T.Y_VELS) if cy.calls[i][3] >= 0)[1]) == blocked_sign and
                   np.sign(cy.winner_vel[1]) == -blocked_sign for cy in hit), bit
    osc = T.STUCK_LEFT | T.STUCK_RIGHT | T.ROTATING_LEFT | T.ROTATING_RIGHT
    assert any(cy.entry_flags & osc and not cy.flags & osc and
               np.hypot(cy.pos[0] - cy.state[0], cy.pos[1] - cy.state[1]) > cy.cfg["oscillation_reset_dist"] for _, _, _, _, cy in every)
    # the two update blocks are not copies: after an in-place winner with thetav > 0 rotating_left stands (first block), after a y_vels
    # winner with vy > 0 strafe_left stands (second block), each from clear flags
    for stage, column, flag in ((T.IN_PLACE, 2, {1.0: T.ROTATING_LEFT, -1.0: T.ROTATING_RIGHT}), (T.Y_VELS, 1, {1.0: T.STRAFE_LEFT, -1.0: T.STRAFE_RIGHT})):
        fresh = {np.sign(cy.winner_vel[column]): cy.flags for _, _, cy in winners(stage) if cy.entry_flags == 0}
        assert fresh == flag, (stage, fresh)
    # ---- modes and limits
    cfgs = [cy.cfg for _, _, _, _, cy in every]
    for key in ("dwa", "holonomic_robot", "heading_scoring", "simple_attractor", "meter_scoring"):
        assert {cfg[key] for cfg in cfgs} == {0, 1}, key
    counts = {(c["cfg"]["vx_samples"], c["cfg"]["vtheta_samples"]) for c, _, _ in cases.values()}
    counts |= {(k["reconfigure"]["vx_samples"], k["reconfigure"]["vtheta_samples"]) for c, _, _ in cases.values() for k in c["cycles"] if k["reconfigure"]}
    assert {(1, 5), (4, 1), (1, 1), (0, 0)} <= counts
    c, _, cycles = cases["sample_counts"]
    assert c["cycles"][2]["reconfigure"]["vx_samples"] == 0 and (cycles[2].cfg["vx_samples"], cycles[2].cfg["vtheta_samples"]) == (1, 1)  # :99-108
    # vtheta_samples = 1: dvtheta is x / 0 (or 0 / 0), the gate of :669 rejects every in-place call, legal and no dearer than the best
    gated = [cy for _, _, _, _, cy in every if cy.cfg["vtheta_samples"] == 1 for i in cy.stage_calls(T.IN_PLACE)
             if 0 <= cy.calls[i][3] <= cy.cost]
    assert gated and all(cy.stage_of(cy.best_call) != T.IN_PLACE for cy in gated)
    # min_in_place_vel_th replaces a smaller sample: five samples over -1 .. 1 have 0 in the middle, and the middle call is -0.4
    assert any(cy.calls[cy.stage_calls(T.IN_PLACE)[2]][2] == -cy.cfg["min_in_place_vel_th"] for _, _, _, _, cy in every
               if cy.cfg["vtheta_samples"] == 5 and (cy.cfg["min_vel_th"], cy.cfg["max_vel_th"]) == (-1.0, 1.0) and not cy.vel.any() and not cy.cfg["dwa"])
    # the gate of :669 reads the unclamped loop variable.  gate_decides: five samples over -1 .. 0.8 (dvtheta = 0.45); the call with
    # +min_in_place_vel_th = 0.6 > dvtheta is made once, for the unclamped 0.35.  It is legal, costs what the winner costs, no stuck flag
    # stands, its lookahead point is on the map and has a strictly smaller goal distance than that of every other in-place call: only
    # the gate, on the unclamped value, can have turned it down (on the clamped value it would let it through)
    c, _, cycles = cases["gate_decides"]
    cy = cycles[0]
    in_place = cy.stage_calls(T.IN_PLACE)
    dvtheta = (cy.cfg["max_vel_th"] - cy.cfg["min_vel_th"]) / (cy.cfg["vtheta_samples"] - 1)
    clamped = [i for i in in_place if cy.calls[i][2] == cy.cfg["min_in_place_vel_th"]]
    assert len(clamped) == 1 and cy.cfg["min_in_place_vel_th"] > dvtheta and cy.entry_flags == 0 and not cy.vel.any()

    def ahead(i):
        x = cy.calls[i][5] + cy.cfg["heading_lookahead"] * np.cos(cy.calls[i][7])
        y = cy.calls[i][6] + cy.cfg["heading_lookahead"] * np.sin(cy.calls[i][7])
        assert _on_map(c, x, y)
        return int(cy.grid[1][int((y - c["origin"][1]) / c["res"]), int((x - c["origin"][0]) / c["res"])])
    assert all(cy.calls[i][3] == cy.cost for i in in_place)
    assert all(ahead(clamped[0]) < ahead(i) for i in in_place if i != clamped[0])
    assert cy.stage_of(cy.best_call) == T.IN_PLACE and cy.best_call != clamped[0] and cy.winner_vel[2] == cy.cfg["max_vel_th"]
    # the final-goal cap: binding where the goal is nearer than max_vel_x * sim_time, and not elsewhere
    def cap(c, k, cy):
        plan = [q["plan"] for q in c["cycles"][:k + 1] if q["plan"] is not None][-1]
        return np.hypot(plan[-1][0] - float(cy.pos[0]), plan[-1][1] - float(cy.pos[1])) / cy.cfg["sim_time"] if len(plan) else np.inf
    caps = [(cap(c, k, cy), cy) for _, c, _, k, cy in every if not cy.entry_flags & T.ESCAPING]
    def fastest(cy):  # the forward grid's last vx_samp, min_vel_x plus dvx added up: max_vel_x to a few ulp
        return max(cy.calls[i][0] for i in cy.stage_calls(T.FORWARD))
    assert any(v < cy.cfg["max_vel_x"] and abs(fastest(cy) - v) < 1e-12 for v, cy in caps)
    assert any(v > cy.cfg["max_vel_x"] and abs(fastest(cy) - cy.cfg["max_vel_x"]) < 1e-12 for v, cy in caps)
    # meter_scoring: reconfigure multiplied the three scales by the resolution
    c, _, cycles = cases["rotate_reconfigure"]
    r = c["cycles"][2]["reconfigure"]
    assert r["meter_scoring"] and [cycles[2].cfg[k] for k in ("pdist_scale", "gdist_scale", "occdist_scale")] == \
        [r[k] * c["res"] for k in ("pdist_scale", "gdist_scale", "occdist_scale")]
    assert cycles[2].entry_flags == cycles[1].flags != 0 and cycles[2].reconfigure  # a reconfigure with persistent state standing
    # ---- heading scoring
    c, m, cycles = cases["heading_bend"]
    plan = c["cycles"][0]["plan"]
    ray = [np.asarray(cycles[0].pos[:2], np.float64) + (plan[-1] - cycles[0].pos[:2]) * t for t in np.linspace(0, 1, 400)]
    assert any(_in_lethal(c, m, x, y) for x, y in ray)  # the last plan pose is out of sight: the scan goes past the first candidate
    assert all(0 < cy.cost < 1e300 for cy in cycles[:3])
    steps = int(cycles[0].calls[0][4])
    assert meta["fleet"]["heading_bend"]["max_sim_steps"] - 2 <= steps  # a call within two steps of the fleet's capacity
    assert [cy.cfg["heading_scoring_timestep"] for cy in cycles[1:]] == [0.1, 0.0, 5.0]
    assert cycles[3].cfg["heading_scoring_timestep"] > cycles[3].cfg["sim_time"]  # beyond the last step: no distances, no heading term
    assert cases["heading_nothing_in_sight"][2][0].cost > 1e300  # 0.3 * DBL_MAX
    # ---- call codes and lengths
    assert {code for _, _, _, _, cy in every for code in cy.calls[:, 3] if code < 0} == {-1.0, -2.0}
    assert any(cy.calls[:, 4].min() == 1 for _, _, _, _, cy in every)  # a one-step call
    c, m, cycles = cases["border"]
    assert not (m[:, -12:] == T.LETHAL).any() and (cycles[0].calls[:, 3] == -1.0).any()  # -1 with nothing to hit: the footprint left the map
    ahead = [(cy.calls[i][5] + cy.cfg["heading_lookahead"] * np.cos(cy.calls[i][7]), cy.calls[i][6] + cy.cfg["heading_lookahead"] * np.sin(cy.calls[i][7]))
             for cy in cycles for i in cy.stage_calls(T.IN_PLACE) if cy.calls[i][3] >= 0]
    assert any(not _on_map(c, x, y) for x, y in ahead) and any(_on_map(c, x, y) for x, y in ahead)
    assert (cases["boxed_in"][2][0].calls[:, 3] == -1.0).all() and (cases["boxed_in"][1] == T.LETHAL).any()  # -1 by collision
    # ---- footprints
    assert {len(c["fp"]) for c, _, _ in cases.values()} >= {2, 4, 5}
    c, m, cycles = cases["lethal_under_robot"]
    under = [i for i in cycles[0].within if m.ravel()[i] == T.LETHAL]
    size = c["size_x"] * c["size_y"]
    assert under and all(cycles[0].grid[0].ravel()[i] < size for i in under) and all(cycles[0].grid[1].ravel()[i] == size for i in under)
    assert cycles[0].pre[0] == -1.0 and cycles[0].cost >= 0  # updatePlan(compute_dists) and scoreTrajectory before any findBestPath
    assert len(cases["vertex_off_map"][2][0].within) < 10 < len(cases["open_forward"][2][0].within)  # returned before the fill
    # the centre cell dearer than every cell under the outline: its cost is what the standing call's occ term holds
    stand = cycles[0].calls[0]
    outline = max(int(v) for v in m.ravel()[cycles[0].within] if v < T.LETHAL and v != 200)
    assert tuple(stand[:3]) == (0.0, 0.0, 0.0) and m.ravel()[cycles[0].within].max() == T.LETHAL and outline < 200
    cx, cy_ = int((cycles[0].pos[0] - c["origin"][0]) / c["res"]), int((cycles[0].pos[1] - c["origin"][1]) / c["res"])
    assert m[cy_, cx] == 200 and stand[3] == cycles[0].cfg["pdist_scale"] * cycles[0].grid[0][cy_, cx] + \
        cycles[0].grid[1][cy_, cx] * cycles[0].cfg["gdist_scale"] + cycles[0].cfg["occdist_scale"] * 200.0
    # four y_vels calls of equal cost: `<=` (:768) lets each one nearer the goal take over, the last wins
    cyc0 = cases["strafe_equal_costs"][2][0]
    ys = cyc0.stage_calls(T.Y_VELS)
    assert len({cyc0.calls[i][3] for i in ys}) == 1 and cyc0.calls[ys[0]][3] >= 0 and cyc0.best_call == ys[-1]
    # ties in the goal distance ahead: the strict `<` (:679, :778) keeps the first of equal calls.  In-place: the first two calls tie at
    # the minimum, same cost; y_vels: every lookahead point lies in the wall, the later calls are cheaper, the first legal one stays
    def ahead_of(c, cy, i):
        x = cy.calls[i][5] + cy.cfg["heading_lookahead"] * np.cos(cy.calls[i][7])
        y = cy.calls[i][6] + cy.cfg["heading_lookahead"] * np.sin(cy.calls[i][7])
        return int(cy.grid[1][int((y - c["origin"][1]) / c["res"]), int((x - c["origin"][0]) / c["res"])])
    ct, _, cyt = cases["ahead_ties"]
    ip = cyt[0].stage_calls(T.IN_PLACE)
    d = [ahead_of(ct, cyt[0], i) for i in ip]
    assert d[0] == d[1] == min(d) and cyt[0].best_call == ip[0] and len({cyt[0].calls[i][3] for i in ip}) == 1
    ct, _, cyt = cases["strafe_ahead_ties"]
    ys = cyt[0].stage_calls(T.Y_VELS)
    assert len({ahead_of(ct, cyt[0], i) for i in ys}) == 1 and cyt[0].best_call == ys[0]
    assert all(0 <= cyt[0].calls[i][3] < cyt[0].calls[ys[0]][3] for i in ys[1:])
    # a two-point footprint whose centre leaves the map
    c2, _, cycles2 = cases["fp2_off_border"]
    assert len(c2["fp"]) == 2 and (cycles2[0].calls[:, 3] == -1.0).any() and (cycles2[0].calls[:, 3] >= 0).any()
    # ---- plans
    c, _, cycles = cases["empty_plan"]
    assert len(c["cycles"][0]["plan"]) == 0 and (cycles[0].calls[:, 3] == -2.0).all()
    assert not _on_map(c, *c["cycles"][2]["plan"][-1]) and cycles[2].cost >= 0
    c, _, cycles = cases["dwa_short_plan"]
    assert len(c["cycles"][2]["plan"]) < len(c["cycles"][0]["plan"])
    c, _, cycles = cases["open_forward"]
    assert c["cycles"][0]["compute_dists"] and len(cycles[0].pre) == 2 and (cycles[0].pre >= 0).all()


def _tp_config(N, cfg, allow_unknown):
    kw = {k: v for k, v in cfg.items() if k != "meter_scoring"}  # the scales are the reference's, after its multiplication
    return N.TpConfig(allow_unknown=allow_unknown, **kw)


def test_oracle_equals_the_reference(golden, orc):
    """Everything equal, bit for bit: both sides are double arithmetic without contraction.  One field, the drive yaw, is bounded: the
    reference hands thetav_ back inside a tf pose (trajectory_planner.cpp:971-975) and its caller reads tf::getYaw of it."""
    from navigation_amd import _lib as N
    g, meta = golden
    drive_yaw_error = 0.0
    for name in meta["cases"]:
      c, costmap, cycles = T.case(g, meta, name)
      for allow_unknown in (c["allow_unknown"], 1 - c["allow_unknown"]):  # no unknown cells: the reference agrees with itself (meta)
        o, plan = None, np.zeros((0, 2))
        for k, cyc in enumerate(cycles):
            where = f"{name} cycle {k} allow_unknown {allow_unknown}"
            if o is None or cyc.reconfigure:  # the oracle has no reconfigure: a new object takes over plan and persistent state
                state = o.state(N.TpState) if o is not None else None
                o = orc.TrajectoryPlanner(costmap, c["res"], _tp_config(N, cyc.cfg, allow_unknown), c["fp"], *c["origin"])
                if state is not None:
                    o.set_state(state)
                    o.update_plan(plan)
            if cyc.plan is not None:
                plan = cyc.plan
                o.update_plan(plan, compute_dists=bool(cyc.compute_dists))
            pos64, vel64 = cyc.pos.astype(np.float64), cyc.vel.astype(np.float64)
            for s, want in zip(cyc.pre_samples, cyc.pre):
                assert o.score_trajectory(pos64, vel64, s) == want, f"{where}: scoreTrajectory{tuple(s)} before findBestPath"
            res, traj, samples = o.find_best_path(cyc.pos, cyc.vel, N.TpResult, N.TpSample)
            for which in range(2):
                assert np.array_equal(o.grid(which), cyc.grid[which].astype(np.float64)), f"{where}: MapGrid {which}"
            assert np.array_equal(o.within_robot(), np.sort(cyc.within)), f"{where}: within_robot cells"
            assert res.n_samples == len(samples) == len(cyc.calls), (where, len(samples), len(cyc.calls))
            assert np.array_equal(np.asarray(samples, np.float64).reshape(-1, 5), cyc.calls[:, :5]), f"{where}: calls (sample, cost_, points)"
            assert np.array_equal(o.call_ends(), cyc.calls[:, 5:8], equal_nan=True), f"{where}: last point of every call"
            assert (res.xv, res.yv, res.thetav, res.cost) == (*cyc.winner_vel, cyc.cost), where
            assert res.best_sample == cyc.best_call and res.n_points == cyc.n_points, (where, res.best_sample, cyc.best_call)
            assert traj.shape == cyc.traj.shape and np.array_equal(traj, cyc.traj), f"{where}: trajectory points"
            st = o.state(N.TpState)
            assert (st.flags, st.prev_x, st.prev_y, st.escape_x, st.escape_y, st.escape_theta) == (cyc.flags, *cyc.state), (where, st.flags, cyc.flags)
            assert list(res.drive)[:2] == list(cyc.drive)[:2], where
            drive_yaw_error = max(drive_yaw_error, abs(res.drive[2] - cyc.drive[2]))
            assert abs(res.drive[2] - cyc.drive[2]) <= DRIVE_YAW_BOUND, where
            for s, (want, ok) in zip(cyc.post_samples, cyc.post):
                got = o.score_trajectory(pos64, vel64, s)
                assert got == want and (got >= 0) == bool(ok), f"{where}: scoreTrajectory / checkTrajectory{tuple(s)}"
    print(f"largest drive yaw difference over the fixture: {drive_yaw_error:.3e}")
