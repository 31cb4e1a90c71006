"""CPU checks of the global-plan yardstick: tests/golden/g13_global_plan.npz regenerates from the reference (its own
orientation_filter.cpp compiled in place) and the CPU oracle; the Python restatement (tests/global_plan_ref.py) applied to the stored
traceback points gives the stored world plans and, per orientation mode, yaws whose half-angle sine and cosine are the reference's
quaternions within 1e-12; and the inputs meet the conditions that make the GPU comparison meaningful."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import global_plan_ref as R  # noqa: E402
import make_global_plan_goldens as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_global_plan.npz")
needs_reference = pytest.mark.skipif(not G.available(), reason="the reference global_planner tree is not on this machine")
SET_VARIANTS = [(s, v) for s, vs in G.SETS.items() for v in vs]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _plans(golden, name, v):
    """per plan that has poses: (case index, start yaw, goal pose, frame, path, world plan, (4, n, 2) quaternions)"""
    key = f"{name}_{v}_"
    old = G.VARIANTS[v].get("old_navfn_behavior", 0)
    at_pose = at_path = 0
    out = []
    for k, n in enumerate(golden[key + "counts"]):
        if n == 0:
            continue
        n_path = int(n) - (2 if old else 1)
        out.append((k, float(golden[name + "_starts"][k][2]), golden[name + "_goals"][k], golden[name + "_frames"][k],
                    golden[key + "path"][at_path:at_path + n_path], golden[key + "plan"][at_pose:at_pose + n],
                    golden[key + "quat"][:, at_pose:at_pose + n]))
        at_pose += int(n)
        at_path += n_path
    assert at_pose == len(golden[key + "plan"]) and at_path == len(golden[key + "path"])
    return out


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path, golden):
    out = tmp_path / "g13.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_global_plan_goldens.py"), "--out", str(out)], check=True, capture_output=True)
    new = np.load(out)
    assert sorted(new.files) == sorted(golden.files)
    for k in golden.files:
        assert np.array_equal(golden[k], new[k]), k


def test_golden_inputs_are_the_tests_inputs(golden):
    for name in G.SETS:
        cases = G.case_set(name)
        assert np.array_equal(golden[name + "_frames"], np.array([c[1] for c in cases], np.float64))
        assert np.array_equal(golden[name + "_starts"], np.array([c[2] for c in cases], np.float64))
        assert np.array_equal(golden[name + "_goals"], np.array([c[3] for c in cases], np.float64))
        for k, c in enumerate(cases):
            assert np.array_equal(golden[name + "_maps"][golden[name + "_map_index"][k]], c[0])
    assert list(golden["batch_default_status"]) == R.batch_cases()[1]
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("name,v", SET_VARIANTS)
def test_restatement_matches_the_reference_filter(golden, name, v):
    old = G.VARIANTS[v].get("old_navfn_behavior", 0)
    worst = 0.0
    for k, start_yaw, goal, frame, path, plan, quat in _plans(golden, name, v):
        poses = R.assemble(path, frame, goal, old)
        assert np.array_equal(poses.view(np.uint64), plan.view(np.uint64)), (name, v, k)
        for mode in range(4):
            if mode == R.FORWARD_THEN_INTERPOLATE and len(poses) < 3:
                continue  # the reference reads before its array; the library's choice (i = 0) has no counterpart
            yaw = R.orientation_filter(poses.copy(), start_yaw, mode)[:, 2]
            d = max(np.abs(np.sin(yaw / 2) - quat[mode, :, 0]).max(), np.abs(np.cos(yaw / 2) - quat[mode, :, 1]).max())
            worst = max(worst, float(d))
            assert d <= 1e-12, (name, v, k, mode, d)
    print(f"{name} {v}: largest quaternion component difference {worst:.3e}")


def test_inputs_meet_their_conditions(golden):
    """n_poses of 2, 3 and 4 and one above 512; the 0.35 search ends at 0, at an interior index and at n - 3; no
    | diff - 0.35 | below 1e-6 (the search's outcome must not hinge on atan2's last bits)."""
    counts, ends, margin = set(), set(), math.inf
    for name, v in SET_VARIANTS:
        old = G.VARIANTS[v].get("old_navfn_behavior", 0)
        for k, start_yaw, goal, frame, path, plan, quat in _plans(golden, name, v):
            n = len(plan)
            counts.add(n)
            info = {}
            R.orientation_filter(R.assemble(path, frame, goal, old), start_yaw, R.FORWARD_THEN_INTERPOLATE, info)
            margin = min(margin, info["margin"])
            if n > 4:
                ends.add("zero" if info["index"] == 0 else "last" if info["index"] == n - 3 else "interior")
                assert 0 <= info["index"] <= n - 3
    assert {2, 3, 4} <= counts and max(counts) > 512, sorted(counts)
    assert ends == {"zero", "interior", "last"}, ends
    assert margin >= 1e-6, margin
    print(f"pose counts {sorted(counts)}; smallest margin {margin:.3e}")


def test_grid_restatement(golden):
    """publishPotential's arithmetic on hand-made arrays: the maximum ignores POT_HIGH, (int8) truncates, max == 0 writes 0."""
    pot = np.array([[0.0, 50.0, 1e10], [199.99, 200.0, 3e10]], np.float32)
    g, mx = R.potential_grid(pot, 100)
    assert mx == np.float32(200.0)
    assert g.tolist() == [[0, 25, -1], [99, 100, -1]]
    g, mx = R.potential_grid(np.array([[0.0, 1e10]], np.float32), 100)
    assert mx == 0 and g.tolist() == [[0, -1]]
    for name, v in SET_VARIANTS:
        grids = golden[f"{name}_{v}_grid"]
        assert grids.dtype == np.int8 and grids.max() <= 100 and (grids == -1).any()


def test_world_to_map_restatement():
    """Costmap2D::worldToMap's edges: the origin itself is cell 0, the far edge is off the map, below the origin is off the map."""
    assert R.costmap_world_to_map(1.0, 2.0, 1.0, 2.0, 0.05, 48, 48) == (0, 0)
    assert R.costmap_world_to_map(1.0 - 1e-9, 2.0, 1.0, 2.0, 0.05, 48, 48) is None
    assert R.costmap_world_to_map(1.0 + 47.99 * 0.05, 2.0, 1.0, 2.0, 0.05, 48, 48) == (47, 0)
    assert R.costmap_world_to_map(1.0 + 48.01 * 0.05, 2.0, 1.0, 2.0, 0.05, 48, 48) is None
    st, sc, gc, s, g = R.endpoints((0.0, 0.0, 0.1), (1.0, 1.0, 0), (2.0, 2.0, 0), 48, 48)
    assert st == R.OK and s == (1.0 / 0.1 - 0.5, 1.0 / 0.1 - 0.5) and sc == (int(1.0 / 0.1), int(1.0 / 0.1))
    assert R.endpoints((0.0, 0.0, 0.1), (0.24, 1.0, 0), (2.0, 2.0, 0), 48, 48)[0] == R.BORDER  # 1.9 cells: inside the start's limit
    assert R.endpoints((0.0, 0.0, 0.1), (1.0, 1.0, 0), (0.14, 2.0, 0), 48, 48)[0] == R.BORDER  # 0.9 cells: inside the goal's
