"""CPU checks of the global_planner yardstick: tests/golden/g18_global_planner_reference.npz is what the reference's own
DijkstraExpansion, AStarExpansion, calculators, GradientPath and GridPath compute (compiled in place by
tools/make_global_planner_goldens.py and driven as planner_core.cpp drives them), the cases reach what they are there for, and
oracle/global_planner_oracle.hpp - what the GPU tests of k_gp_plan compare with - reproduces it bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import global_plan_ref as R  # noqa: E402
import global_planner_reference_cases as T  # noqa: E402
import make_global_planner_goldens as M  # noqa: E402
from test_goldens import G8_VARIANTS  # noqa: E402
from test_navfn import GP_WF_VARIANTS  # noqa: E402

needs_reference = pytest.mark.skipif(not M.available(), reason="the reference global_planner / costmap_2d trees are not on this machine")
HIGH = 1e9  # "below POT_HIGH", with room


@pytest.fixture(scope="module")
def golden():
    return T.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path):
    out = tmp_path / "g18.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_global_planner_goldens.py"), "--out", str(out)], check=True, capture_output=True)
    new, old = np.load(out), np.load(T.GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = old[k], new[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert (np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)), k


def test_golden_is_no_larger_than_the_largest_fixture():
    golden_dir = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(T.GOLDEN) <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if not f.startswith("g18_"))


def test_golden_holds_the_cases_of_the_cases_module(golden):
    plans, meta = golden
    cases = T.cases()
    assert meta["n_cases"] == len(plans) == len(cases) and len({p.name for p in plans}) == len(plans)
    for p, c in zip(plans, cases):
        assert p.name == c["name"] and np.array_equal(p.cmap, c["cmap"]) and p.params == T.full_params(c["params"])
        assert tuple(p.start) == c["start"] and tuple(p.goal) == c["goal"] and tuple(p.goal_cell) == T.goal_cell(c)


# ------------------------------------------------------------------------------------------------ what the cases are there for
def _beside(mask):
    """cells with a 4-neighbour in mask"""
    out = np.zeros_like(mask)
    out[1:, :] |= mask[:-1, :]
    out[:-1, :] |= mask[1:, :]
    out[:, 1:] |= mask[:, :-1]
    out[:, :-1] |= mask[:, 1:]
    return out


def _enterable(p):
    """the cells the expander may give a potential: DijkstraExpansion::getCost below lethal_cost (dijkstra.h:86-95), AStarExpansion::add's
    test (astar.cpp:87)"""
    c, pr = p.seen.astype(np.int32), p.params
    unknown = (c == 255) & bool(pr["allow_unknown"])
    return ((c < pr["lethal_cost"] - 1) if pr["use_dijkstra"] else (c < pr["lethal_cost"])) | unknown


def test_cases_reach_what_they_are_for(golden):
    """Each condition from the inputs and the recorded results alone.  Not reachable on maps of this size, and not claimed: the
    10 000-entry cap of the priority buffers (a front of 10 000 cells needs a map of millions)."""
    plans, _ = golden
    dij = [p for p in plans if p.params["use_dijkstra"]]
    ast = [p for p in plans if not p.params["use_dijkstra"]]
    # ---- shapes and end points
    shapes = {p.cmap.shape for p in plans}
    assert all(24 <= min(s) and max(s) <= 64 for s in shapes)
    assert sum(s[0] != s[1] for s in shapes) >= 2 and any(s[1] % 2 for s in shapes)
    for p in plans:
        ny, nx = p.cmap.shape
        for x, y in (p.start, p.goal):  # three cells from every edge: the goal's 5 x 5 block stays off the border rows, and the mirrored
            assert 3 <= int(x) <= nx - 4 and 3 <= int(y) <= ny - 4, p.name  # end points of the GPU test's neighbour plans are legal too
        assert tuple(p.goal_cell) == (int(p.goal[0]), int(p.goal[1]))
    # ---- parameter sets
    have = [p.params for p in plans]
    for kw in list(G8_VARIANTS) + list(GP_WF_VARIANTS):
        assert T.full_params(kw) in have, kw
    for quadratic in (0, 1):
        assert any(p.params["neutral_cost"] > 50 and p.params["use_quadratic"] == quadratic for p in dij)
        assert any(p.params["neutral_cost"] < 50 and p.params["use_quadratic"] == quadratic for p in dij)
    assert any(p.params["lethal_cost"] == 255 for p in dij) and any(195 <= p.params["lethal_cost"] <= 205 for p in dij)
    bare = [p for p in plans if not p.params["outline_map"]]
    assert bare and all((np.concatenate([p.cmap[0], p.cmap[-1], p.cmap[:, 0], p.cmap[:, -1]]) == 254).all() for p in bare)
    assert all(p.found_legal and p.path_ret == 1 for p in bare)

    # ---- both expanders: nothing but enterable cells (and the start's own seeds) holds a potential before clearEndpoint; beside
    # reached cells lie cells of every cost that must stay out, and of the two that must come in
    def beside_reached(p, cost):
        reached = p.potential_before < HIGH
        return (p.seen == cost) & _beside(reached) & ~p.goal_block

    for p in plans:
        reached = p.potential_before < HIGH
        seeds = np.zeros(p.cmap.shape, bool)
        seeds[int(p.start[1]):int(p.start[1]) + 2, int(p.start[0]):int(p.start[0]) + 2] = True
        assert not (reached & ~_enterable(p) & ~seeds).any(), p.name
    for group, last_in in ((dij, 2), (ast, 1)):  # Dijkstra enters up to lethal - 2, A* up to lethal - 1
        lethals = {p.params["lethal_cost"] for p in group} if group is dij else {253}
        assert lethals >= {253, 255}.intersection(lethals | ({255} if group is dij else set()))
        for lethal in lethals:
            g = [p for p in group if p.params["lethal_cost"] == lethal]
            assert g
            assert any((p.potential_before[beside_reached(p, lethal - last_in)] < HIGH).any() for p in g), lethal       # the last cost that enters
            for cost in sorted({lethal - last_in + 1, lethal, 254}):                                                      # stay out
                if cost == 255:
                    continue  # (lethal_cost 255: 255 is the unknown value, below)
                assert any(beside_reached(p, cost).any() for p in g), (lethal, cost)
                assert not any((p.potential_before[p.seen == cost] < HIGH).any() for p in g), (lethal, cost)
        assert any(p.params["allow_unknown"] and (p.potential_before[beside_reached(p, 255)] < HIGH).any() for p in group)   # unknown, allowed
        known = [p for p in group if not p.params["allow_unknown"]]
        assert any(beside_reached(p, 255).any() for p in known) and not any((p.potential_before[p.seen == 255] < HIGH).any() for p in known)
    # ---- Dijkstra: a goal several priority steps up; the getCost clamp
    assert any(p.potential_before[p.goal_cell[1], p.goal_cell[0]] > p.params["lethal_cost"] + 3 * 100 for p in dij if p.found_legal)

    def clamped(p):
        c = p.seen.astype(np.float32)
        v = c * np.float32(p.params["cost_factor"]) + np.float32(p.params["neutral_cost"])
        return _enterable(p) & (v >= p.params["lethal_cost"]) & ~p.goal_block
    assert any((p.potential_before[clamped(p)] < HIGH).any() for p in dij)
    # ---- precise start: an offset of .995 or more rounds to 1 (the seeds to its right are 0), an integral start (three seeds 0)
    precise = [p for p in dij if not p.params["old_navfn_behavior"]]

    def seeds_of(p):
        x, y = int(p.start[0]), int(p.start[1])
        return p.potential_before[y, x], p.potential_before[y, x + 1], p.potential_before[y + 1, x], p.potential_before[y + 1, x + 1]
    up = [p for p in precise if p.start[0] - int(p.start[0]) >= 0.995 and 0.1 < p.start[1] - int(p.start[1]) < 0.9]
    assert up and all(s[1] == 0 and s[3] == 0 and s[0] > 0 and s[2] > 0 for s in map(seeds_of, up))
    whole = [p for p in precise if p.start[0] == int(p.start[0]) and p.start[1] == int(p.start[1])]
    assert whole and all(s[0] == 0 and s[1] == 0 and s[2] == 0 for s in map(seeds_of, whole))
    assert any(0.005 < p.start[0] - int(p.start[0]) < 0.995 and 0.005 < p.start[1] - int(p.start[1]) < 0.995 for p in precise)
    # ---- A*: costs + neutral_cost past 255 (narrowed to unsigned char), an open area, GradientPath failing after a legal potential
    assert any(p.params["neutral_cost"] == 50 and (p.potential_before[(p.seen >= 206) & (p.seen <= 252) & (p.seen < p.params["lethal_cost"]) &
                                                                      ~p.goal_block] < HIGH).any() for p in ast)
    assert any(p.found_legal and p.path_ret == 1 and not p.seen[1:-1, 1:-1].any() for p in ast)
    gradient_ast = [p for p in ast if not p.params["use_grid_path"] and p.found_legal]
    assert any(p.path_ret == 1 for p in gradient_ast)

    # The two ways it fails, both recorded: the walk stops short on a zero gradient, or circles until its 4 * ns limit.  (Not a
    # third, `int minp = potential[stc]` of 1e10 at gradient_path.cpp:123: stc never holds POT_HIGH in getPath once a legal potential
    # was found.  It starts on the goal cell, which has one; a gradient step moves it within the nine cells just tested finite; a
    # grid step moves it to a neighbour of lower, hence finite, potential.  No case can reach that conversion.)
    assert any(p.path_ret == 0 and 0 < p.path_len < p.cmap.size for p in gradient_ast)
    assert any(p.path_ret == 0 and p.path_len == 4 * p.cmap.size for p in gradient_ast)
    # ---- clearEndpoint: in the goal's block, cells the expansion had not reached - free, 206 and more, a 254 and a 255 - all given a potential
    for group in (dij, ast):
        def filled(p, lo, hi):
            m = p.goal_block & (p.potential_before >= HIGH) & (p.seen >= lo) & (p.seen <= hi)
            return m.any() and (p.potential[m] < HIGH).all()
        assert any(not p.params["old_navfn_behavior"] and p.found_legal and filled(p, 0, 0) and filled(p, 206, 253) and filled(p, 254, 254) and
                   filled(p, 255, 255) for p in group)
    old = [p for p in plans if p.params["old_navfn_behavior"]]
    assert old and all(np.array_equal(bits(p.potential), bits(p.potential_before)) for p in old)  # no clearEndpoint there
    # ---- GradientPath
    arrived = [p for p in plans if not p.params["use_grid_path"] and p.path_ret == 1]

    def grid_points_beside_high(p):
        whole = (p.path == np.floor(p.path)).all(axis=1)
        whole[[0, -1]] = False
        near = [(p.potential[int(y) - 2:int(y) + 3, int(x) - 2:int(x) + 3] >= HIGH).any() for x, y in p.path[whole]]
        return (~whole[1:-1]).any() and any(near)  # gradient steps too
    assert any(grid_points_beside_high(p) for p in arrived if p.params["use_dijkstra"])
    assert any(((p.path[2:] == p.path[:-2]).all(axis=1)).any() for p in arrived if p.params["use_dijkstra"])  # the oscillation test fires
    assert any(p.path_len > 150 for p in arrived)
    assert all(np.array_equal(p.path[-1], np.asarray(p.start, np.float32)) for p in arrived)
    # ---- not found: both expanders, and no traceback then
    for group in (dij, ast):
        assert any(not p.found_legal for p in group)
    assert all(p.path_ret == -1 and p.path_len == 0 for p in plans if not p.found_legal)


# ------------------------------------------------------------------------------------------------ the oracle against the fixture
def test_oracle_reproduces_the_reference(orc, golden):
    plans, _ = golden
    wrong = []
    for p in plans:
        o = orc.global_planner_plan_trace(p.cmap, p.start, p.goal, p.goal_cell, **p.params)
        what = []
        if o["found_legal"] != p.found_legal:
            what.append(f"found_legal {o['found_legal']} != {p.found_legal}")
        for key in ("potential_before", "potential"):
            d = bits(o[key]) != bits(getattr(p, key))
            if d.any():
                j, i = np.argwhere(d)[0]
                what.append(f"{key}: {d.sum()} cells differ, first ({i}, {j}): {o[key][j, i]!r} != {getattr(p, key)[j, i]!r} (cost {p.seen[j, i]})")
        if o["path_ret"] != p.path_ret or len(o["path"]) != p.path_len:
            what.append(f"traceback returned {o['path_ret']} with {len(o['path'])} points, the reference {p.path_ret} with {p.path_len}")
        elif not np.array_equal(bits(o["path"]), bits(p.path)):
            i = np.nonzero((bits(o["path"]) != bits(p.path)).any(axis=1))[0][0]
            what.append(f"path point {i}: {o['path'][i]} != {p.path[i]}")
        if what:
            wrong.append(p.name + ": " + "; ".join(what))
    assert not wrong, "\n".join(wrong)


def test_oracle_plan_agrees_with_its_trace(orc, golden):
    """global_planner_plan - what every GPU test calls - is the same run: its path is the trace's where the traceback arrived, empty otherwise"""
    plans, _ = golden
    for p in plans:
        path, pot, legal, _ = orc.global_planner_plan(p.cmap, p.start, p.goal, p.goal_cell, **p.params)
        assert int(legal) == p.found_legal and np.array_equal(bits(pot), bits(p.potential)), p.name
        assert len(path) == (p.path_len if p.path_ret == 1 else 0) and (p.path_ret != 1 or np.array_equal(bits(path), bits(p.path))), p.name


@needs_reference
def test_reference_reproduces_the_end_to_end_fixture(tmp_path):
    """tests/golden/g13_global_plan.npz stores the oracle's traceback points of its `batch` plans (S_V_path); the reference's classes,
    run on the same inputs through the harness, give the same points bit for bit - so that fixture is the reference's as well."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_global_plan.npz"))
    exe = M.build_harness(str(tmp_path))
    from make_global_plan_goldens import SETS, VARIANTS

    def core(cm, s, g_, gc, **kw):
        c = dict(cmap=cm, params=kw)
        r = M.run_harness(exe, str(tmp_path), [(T.outlined(c), T.full_params(kw), s, g_, gc)])[0]
        return (r["path"] if r["path_ret"] == 1 else np.zeros((0, 2), np.float32)), r["potential"]
    cases = [(g["batch_maps"][g["batch_map_index"][k]], g["batch_frames"][k], g["batch_starts"][k], g["batch_goals"][k])
             for k in range(len(g["batch_starts"]))]
    for v in SETS["batch"]:
        refs = [R.make_plan(core, *c, R.NONE, **VARIANTS[v]) for c in cases]
        assert np.array_equal(np.array([r["status"] for r in refs], np.int32), g[f"batch_{v}_status"]), v
        path = np.concatenate([r["path"] for r in refs if r["n_poses"]]).astype(np.float32)
        assert np.array_equal(bits(path), bits(g[f"batch_{v}_path"])), v
