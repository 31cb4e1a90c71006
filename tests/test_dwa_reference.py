"""CPU checks of the DWA scoring yardstick: tests/golden/g15_dwa_reference.npz is what the reference's own DWAPlanner, generator,
critics and SimpleScoredSamplingPlanner compute (compiled in place by tools/make_dwa_goldens.py), the fixture covers the branches
the scoring kernels take, and oracle/planner_oracle.hpp - what every GPU test of k_score_*, k_samples and k_select compares with -
reproduces it bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dwa_reference_cases as D  # noqa: E402
import make_dwa_goldens as M  # noqa: E402

DRIVE_YAW_BOUND = 2e-15  # 4.5 ulp of pi, see test_oracle_equals_the_reference

needs_reference = pytest.mark.skipif(not M.available(), reason="the reference local-planner trees are not on this machine")


@pytest.fixture(scope="module")
def golden():
    return D.load()


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path):
    out = tmp_path / "g15.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_dwa_goldens.py"), "--out", str(out)], check=True, capture_output=True)
    new, old = np.load(out), np.load(D.GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = old[k], new[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), k
        else:
            assert np.array_equal(a, b), k
    assert os.path.getsize(D.GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
                                            for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if not f.startswith("g15_"))


def _longest_edge(fp):
    return max(float(np.hypot(*(fp[i] - fp[(i + 1) % len(fp)]))) for i in range(len(fp)))


def test_golden_cases_cover_the_branches(golden):
    g, meta = golden
    cases = {n: D.case(g, meta, n) for n in meta["cases"]}
    assert set(meta["sets"].values()) == {"sweep", "gen"}
    codes = {name: set() for name in D.CRITICS}
    for kset in ("sweep", "gen"):
        rejected = collided = valid = no_winner = flags = 0
        chunks, vertices, steps = set(), set(), set()
        for name, (c, _, cycles, _) in cases.items():
            if c["set"] != kset:
                continue
            cfg = c["cfg"]
            sweep = bool(cfg["use_dwa"] and cfg["discretize_by_time"] and len(c["fp"]) <= 8 and
                         int(np.ceil(cfg["sim_time"] / cfg["sim_granularity"])) <= 127 and not any(c["agg"]) and not any(c["yshift"]))
            assert sweep == (kset == "sweep"), name
            e = _longest_edge(c["fp"])
            chunks.add(0 if e <= 0.25 else 1 if e <= 0.4 else 2 if e <= 0.55 else 3)
            vertices.add(len(c["fp"]))
            for cyc in cycles:
                acc = cyc.accepted
                rejected += int((~acc).sum())
                collided += int((cyc.total_full[acc] < 0).sum())
                valid += int((cyc.total_full[acc] >= 0).sum())
                no_winner += int(not cyc.found)
                flags += int(cyc.flags != 0)
                steps |= set(cyc.slot_points[acc].tolist())
                for i, critic in enumerate(D.CRITICS):
                    col = cyc.critic[acc][:, i]
                    codes[critic] |= set(col[col < 0].tolist())
                assert cyc.found == (cyc.best_index >= 0) and np.isnan(cyc.total_full[~acc]).all()
        assert rejected and collided and valid and no_winner and flags, kset
        assert chunks == {0, 1, 2, 3}, (kset, chunks)  # every footprint-edge instantiation of the scoring kernels
        if kset == "sweep":
            assert {3, 4, 5, 8} <= vertices and 10 in steps and 120 <= max(steps) <= 127
        else:
            assert 9 in vertices and max(steps) > 127 and len(steps) > 8  # per-sample step counts
    # every failure code a critic can return through this wiring: the oscillation critic knows -5 only, the obstacle critic's -7
    # (centre off the map) and -9 (no footprint) lie behind its -6, goal_front and alignment do not stop on failure, so -4 is theirs
    assert codes["oscillation"] == {-5.0} and codes["obstacle"] == {-6.0}
    assert codes["goal_front"] == {-4.0} and codes["alignment"] == {-4.0}
    assert codes["path"] == {-2.0, -3.0, -4.0} and codes["goal"] == {-2.0, -3.0, -4.0}
    cfgs = [c["cfg"] for c, _, _, _ in cases.values()]
    for key, values in (("use_dwa", {0, 1}), ("discretize_by_time", {0, 1}), ("sum_scores", {0, 1}), ("allow_unknown", {0, 1})):
        assert {cfg[key] for cfg in cfgs} == values, key
    for key in ("occdist_scale", "path_distance_bias", "goal_distance_bias", "forward_point_distance"):
        assert any(cfg[key] == 0.0 for cfg in cfgs), key
    assert {cfg["cheat_factor"] for cfg in cfgs} >= {0.25, 1.0, 4.0}
    assert any((cfg["vx_samples"], cfg["vy_samples"], cfg["vth_samples"]) == (3, 10, 20) for cfg in cfgs)
    aggs = {(m, D.AGGREGATIONS[a]) for c, _, _, _ in cases.values() for m, a in zip(D.MAP_GRID_CRITICS, c["agg"]) if a}
    assert {a for _, a in aggs} == {"sum", "product"} and any(y != 0.0 for c, _, _, _ in cases.values() for y in c["yshift"])
    # no NO_INFORMATION cells: the reference's answer for them hangs on an uninitialised read (dwa_reference_cases.build_cases)
    assert not any((m == D.NOINFO).any() for _, m, _, _ in cases.values())
    # alignment switched off near the goal, and on for the same plan with a smaller cheat_factor
    assert cases["gen_short_plan_cheat4"][2][0].scale[3] == 0.0 and cases["gen_short_plan_cheat025"][2][0].scale[3] > 0.0
    assert len(cases["gen_short_plan_cheat4"][2][0].plan) == 12
    # zero scales reach the critics: the reference then skips them
    assert cases["gen_noocc"][2][0].scale[1] == 0.0 and cases["gen_long_nopath"][2][0].scale[4] == 0.0
    # a plan that leaves the map, a goal cell that is lethal
    c, m, cycles, _ = cases["gen_noocc"]
    assert (cycles[0].plan[:, 0] >= c["size_x"] * c["res"]).any()
    c, m, cycles, _ = cases["gen_lethal_goal"]
    gx, gy = (cycles[0].plan[-1] / c["res"]).astype(int)
    assert m[gy, gx] == D.LETHAL and not cycles[0].found
    # oscillation: flags set, standing for a third cycle (with -5 samples), reset by distance, set again, reset by angle
    for name in ("sweep_oscillation", "gen_oscillation"):
        cyc = cases[name][2]
        assert [bool(x.flags & 0x100) for x in cyc] == [False, True, True, False, False, True, False], name
        assert (cyc[2].critic[cyc[2].accepted][:, 0] == -5.0).any()
        assert np.hypot(*(cyc[3].pos[:2] - cyc[2].pos[:2])) > 0.05 and cyc[3].pos[2] == cyc[2].pos[2]
        assert np.array_equal(cyc[6].pos[:2], cyc[5].pos[:2]) and abs(cyc[6].pos[2] - cyc[5].pos[2]) > 0.2
    # checkTrajectory: legal, colliding and generator-rejected samples (the reference passes what its generator rejects: no points)
    c, _, cycles, ok = cases["gen_defaults"]
    assert ok.any() and not ok.all() and ok[list(map(tuple, c["checks"])).index((np.float32(0.9), 0.0, 0.0))]
    # the DWAPlanner wiring where it can be driven, the restated one only where DWAPlanner cannot pass the argument
    for name, (c, _, _, _) in cases.items():
        direct = bool(c["cfg"]["discretize_by_time"] or any(c["agg"]) or any(c["yshift"]))
        assert meta["wiring"][name] == ("direct" if direct else "DWAPlanner"), name
    assert meta["rollout_trig"] == 0 and meta["rollout_trig_probe_states_that_tell_the_modes_apart"] >= 5


def test_rollout_trig_of_the_reference_build(golden):
    """computeNewPositions as the reference build compiled it equals the double-trig form (rollout_trig = 0) on every probe state, and
    the float form differs on some: the fixture's meta entry is what the probe says."""
    g, meta = golden
    mode, differ = D.trig_mode(g["trig_probe_in"].astype(np.float64), g["trig_probe_out"].astype(np.float64))
    assert mode == meta["rollout_trig"] and differ == meta["rollout_trig_probe_states_that_tell_the_modes_apart"]


def _oracle_planner(orc, c, costmap):
    cfg = dict(c["cfg"])
    p = orc.DwaPlanner(costmap, c["res"], 0.0, 0.0, orc.DwaConfig(**cfg))
    for m, a, y in zip(D.MAP_GRID_CRITICS, c["agg"], c["yshift"]):
        if a or y:
            p.set_map_grid_options(m, D.AGGREGATIONS[a], y)
    return p


def test_oracle_equals_the_reference(golden, orc):
    """Everything equal, bit for bit: both sides are double arithmetic without contraction.  One field, the drive yaw, is bounded."""
    g, meta = golden
    drive_yaw_error = [0.0]
    for name in meta["cases"]:
        c, costmap, cycles, check_ok = D.case(g, meta, name)
        c["cfg"]["rollout_trig"] = meta["rollout_trig"]
        p = _oracle_planner(orc, c, costmap)
        for k, cyc in enumerate(cycles):
            where = f"{name} cycle {k}"
            if cyc.set_plan:
                p.set_plan()
            res, traj, cref, cfull, status = p.cycle(cyc.pos, cyc.vel, cyc.plan, c["fp"])
            for which in range(3):
                assert np.array_equal(p.grid(which), cyc.grid[which].astype(np.float64)), f"{where}: MapGrid {which}"
            assert res.n_samples == cyc.n_slots, where
            assert np.array_equal(p.samples().view(np.uint32), cyc.samples.view(np.uint32)), f"{where}: sample velocities"
            acc = cyc.accepted
            assert np.array_equal(status == 1, acc), f"{where}: accept mask"
            assert np.array_equal(cfull[acc], cyc.total_full[acc]), f"{where}: totals and failure codes"
            assert np.array_equal(cref[acc], cyc.total_ref[acc]), f"{where}: totals with the early-out"
            assert res.n_scored == int(acc.sum()) and res.n_valid == int((cyc.total_full[acc] >= 0).sum()), where
            assert res.best_index == cyc.best_index, where
            assert res.oscillation_flags == cyc.flags, where
            flags, prev = p.oscillation()
            assert flags == cyc.flags and np.array_equal(prev, cyc.prev), f"{where}: oscillation state"
            # drive yaw: the one field computed in another order.  The reference hands thetav back inside a tf pose (dwa_planner.cpp:363-367)
            # and its caller reads tf::getYaw of it: a yaw -> quaternion -> yaw round trip of double sin / cos / atan2, a few ulp of a
            # value below pi; the oracle (and the library) return thetav itself.  DRIVE_YAW_BOUND is 4.5 ulp of pi; measured: DESIGN 4n.
            assert list(res.drive)[:2] == list(cyc.drive)[:2], where
            drive_yaw_error[0] = max(drive_yaw_error[0], abs(res.drive[2] - cyc.drive[2]))
            assert abs(res.drive[2] - cyc.drive[2]) <= DRIVE_YAW_BOUND, where
            if cyc.found:
                assert (res.xv, res.yv, res.thetav) == tuple(np.float32(v) for v in cyc.winner_vel), where
                assert res.cost == cyc.cost, where
                assert traj.shape == cyc.traj.shape and np.array_equal(traj, cyc.traj), f"{where}: trajectory points"
            else:
                assert res.cost < 0, where
        last = cycles[-1]
        for sample, ok in zip(c["checks"], check_ok):
            assert p.check_trajectory(last.pos, last.vel, sample) == bool(ok), f"{name}: checkTrajectory{tuple(sample)}"
    print(f"largest drive yaw difference over the fixture: {drive_yaw_error[0]:.3e}")
