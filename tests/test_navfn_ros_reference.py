"""CPU checks of the navfn_ros yardstick: tests/golden/g14_navfn_ros.npz regenerates from the reference (its own navfn.cpp compiled in
place and driven as NavfnROS::makePlan drives it); the Python restatement (tests/navfn_ros_ref.py) on the CPU oracle's NavFn gives
the stored potentials, best cells, second paths and statuses bit for bit - which pins the oracle's NavFn, and the claim that the
gradients memoised by the expansion's calcPath do not change the second path, against the real code; and the window search equals a
literal transcription of the reference's loops on its edge cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import navfn_ros_ref as R  # noqa: E402
import make_navfn_ros_goldens as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_navfn_ros.npz")
needs_reference = pytest.mark.skipif(not G.available(), reason="the reference navfn tree is not on this machine")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path, golden):
    out = tmp_path / "g14.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_navfn_ros_goldens.py"), "--out", str(out)], check=True, capture_output=True)
    new = np.load(out)
    assert sorted(new.files) == sorted(golden.files)
    for k in golden.files:
        assert golden[k].tobytes() == new[k].tobytes(), k


def test_golden_inputs_are_the_tests_inputs(golden):
    for name in G.SETS:
        cases = G.case_set(name)
        assert np.array_equal(golden[name + "_frames"], np.array([c[1] for c in cases], np.float64))
        assert np.array_equal(golden[name + "_starts"], np.array([c[2] for c in cases], np.float64))
        assert np.array_equal(golden[name + "_goals"], np.array([c[3] for c in cases], np.float64))
        assert np.array_equal(golden[name + "_tolerances"], np.array([c[4] for c in cases], np.float64))
        assert np.array_equal(golden[name + "_weights"], np.array([c[5:7] for c in cases], np.float64))
        for k, c in enumerate(cases):
            assert np.array_equal(golden[name + "_maps"][golden[name + "_map_index"][k]], c[0])
    assert list(golden["batch_status"]) == R.batch_cases()[1]
    assert os.path.getsize(GOLDEN) < 256 * 1024


@pytest.mark.parametrize("name", G.SETS)
def test_restatement_on_the_oracle_matches_the_reference(orc, golden, name):
    cases = G.case_set(name)
    attempted = list(golden[name + "_attempted"])
    at = 0
    for k, c in enumerate(cases):
        r = R.make_plan(orc, *c)
        assert r["status"] == golden[name + "_status"][k], (name, k, r["status"])
        n = int(golden[name + "_path_len"][k])
        ref_path = golden[name + "_path"][at:at + n]
        at += n
        if k not in attempted:
            assert r["goal_cell"] is None and n == 0
            continue
        assert np.array_equal(r["potential"].view(np.uint32), golden[name + "_potential"][attempted.index(k)].view(np.uint32)), (name, k)
        assert bool(golden[name + "_found"][k]) == r["found"] and golden[name + "_candidates"][k] == r["candidates"], (name, k)
        b = r["best"]
        assert tuple(golden[name + "_best_cell"][k]) == (tuple(b["cell"]) if b else (-1, -1)), (name, k)
        if b:
            want = np.array([b["x"], b["y"], b["cost"]])
            got = np.array(list(golden[name + "_best_xy"][k]) + [golden[name + "_best_cost"][k]])
            assert want.tobytes() == got.tobytes(), (name, k)
        if golden[name + "_path_ret"][k]:
            assert np.array_equal(r["path"].view(np.uint32), ref_path.view(np.uint32)), (name, k)
            assert r["n_poses"] == n + 1
        else:
            # The walk failed in the reference (calcPath returned 0).  Its getPlanFromPotential reads getPathLen(), the points walked
            # so far, and makes a plan of them; the restatement and the library report NO_PLAN, as navgpu_navfn_path reports no path.
            # Those points are the first n of the oracle's unlimited walk: calcPath's steps do not depend on its limit.
            assert r["n_poses"] == 0 and len(r["path"]) == 0
            if b:
                unlimited = orc.navfn_calc_path(r["potential"], r["start_cell"], b["cell"])
                assert len(unlimited) == 0 or np.array_equal(unlimited[:n].view(np.uint32), ref_path.view(np.uint32)), (name, k)
    assert at == len(golden[name + "_path"])


def test_serpentine_is_beyond_the_second_walks_limit(orc, golden):
    cm, frame, s, g = R.serpentine_case()
    r = R.make_plan(orc, cm, frame, s, g, 0.0)
    unlimited = orc.navfn_calc_path(r["potential"], r["start_cell"], r["goal_cell"])
    assert r["found"] and r["candidates"] == 1 and len(unlimited) > 4 * 64 and r["status"] == R.NO_PLAN
    assert golden["serpentine_path_ret"][0] == 0 and golden["serpentine_path_len"][0] == 4 * 64 and golden["serpentine_found"][0] == 1


def _loops_agree(pot, frame, goal, tol, w=(1.0, 0.0)):
    cand, best = R.window_search(pot, frame, goal, tol, *w)
    found, cost, pose = R.window_search_loops(pot, frame, goal, tol, *w)
    assert found == (best is not None)
    if best:
        assert (best["x"], best["y"]) == pose and best["cost"] == cost
    return cand, best


def test_window_edge_cases_match_the_literal_loops():
    rs = np.random.RandomState(5)
    pot = np.where(rs.random_sample((48, 48)) < 0.3, np.float32(R.POT_HIGH), rs.uniform(0, 3000, (48, 48)).astype(np.float32))
    pot[0, :] = pot[-1, :] = pot[:, 0] = pot[:, -1] = np.float32(R.POT_HIGH)
    frame = (-1.2, 0.7, 0.05)
    centre = R.cell_pose(frame, (20, 21), 0)[:2]
    pot[21, 20] = 7.0
    for w in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.01), (0.0, 0.0)):
        assert _loops_agree(pot, frame, centre, 0.0, w)[0] == 1          # tol = 0: one candidate, the goal's own cell
        assert _loops_agree(pot, frame, centre, -0.1, w) == (0, None)    # tol < 0: no iteration
        assert _loops_agree(pot, frame, centre, float("nan"), w) == (0, None)
        assert _loops_agree(pot, frame, centre, 0.33, w)[0] > 50
        # windows hanging off the map on each side, and wholly off it
        for cell in ((1, 20), (46, 20), (20, 1), (20, 46), (1, 1), (46, 46)):
            cand, best = _loops_agree(pot, frame, R.cell_pose(frame, cell, 0)[:2], 0.3, w)
            assert cand > 0 and best is not None
        assert _loops_agree(pot, frame, [frame[0] - 1.0, frame[1] + 1.0], 0.3, w) == (0, None)
        cand, _ = _loops_agree(pot, frame, [frame[0] - 0.1, frame[1] + 1.0], 0.3, w)
        assert cand > 0
    # all weights zero: every candidate costs 0 and the first in scan order wins
    cand, best = _loops_agree(pot, frame, centre, 0.2, (0.0, 0.0))
    assert best["cost"] == 0.0 and best["index"] == min(
        iy * 9 + ix for iy, y in enumerate(R.window_sequence(centre[1], 0.2, 0.05)) for ix, x in enumerate(R.window_sequence(centre[0], 0.2, 0.05))
        if R.point_potential(pot, frame, x, y) < R.POT_HIGH)
    # exact ties on the ring (power-of-two resolution: exact sums): the lowest scan index
    cm, rframe, _, rg, rtol = R.ring_case()
    flat = np.full((48, 48), np.float32(100.0))
    flat[26:31, 28:33] = np.float32(R.POT_HIGH)
    cand, best = _loops_agree(flat, rframe, rg, rtol)
    assert best["cell"] == (30, 25) and best["cost"] == 3 * rframe[2] and cand == 81 - 25
    # an infinite cost never wins (inf is not < DBL_MAX); a NaN cost neither
    cand, best = _loops_agree(flat, rframe, rg, rtol, (float("inf"), 0.0))
    assert cand == 56 and best is None
    assert _loops_agree(flat, rframe, rg, rtol, (float("nan"), 1.0))[1] is None


def test_world_to_map_and_sequences():
    assert R.window_sequence(1.0, 0.0, 0.05) == [1.0]
    assert R.window_sequence(1.0, -0.5, 0.05) == [] and R.window_sequence(1.0, float("nan"), 0.05) == []
    seq = R.window_sequence(0.3, 0.25, 0.05)
    p, want = 0.3 - 0.25, []
    while p <= 0.3 + 0.25:
        want.append(p)
        p += 0.05
    assert seq == want and len(seq) in (10, 11)
    with pytest.raises(AssertionError):
        R.window_sequence(0.0, 4097 * 0.05 / 2, 0.05)
