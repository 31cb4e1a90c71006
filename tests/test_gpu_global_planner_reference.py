"""k_gp_plan (DijkstraExpansion / AStarExpansion in reference order, clearEndpoint, GradientPath / GridPath, one lane per plan) against
the reference's own numbers: tests/golden/g18_global_planner_reference.npz, written by tools/make_global_planner_goldens.py from
global_planner's classes compiled in place and driven as planner_core.cpp drives them.  Reads the fixture only: no reference tree, no
CPU oracle.  Needs a real MI355X.

Bar: bit equality of potential(k) with the array after clearEndpoint, of found with "the traceback arrived", of path_length and of
path(k) (nothing where the traceback did not arrive: the library reports no path then, as getPlanFromPotential makes no plan).

Every case runs through NavFn.global_planner_plan on a handle of three plans, the case in the middle.  Its neighbours are the same map
mirrored in y (plan 0) and in x (plan 2) with the end points' cells mirrored alike: other costs, other cells, so a batch-indexing
error shows in the middle plan.

For the Dijkstra cases the tiled wavefront (wavefront=True) is held to the same reference-order array by the contract of
tests/test_navfn.py's _check_gp_wavefront, with its number: outside the goal's 5 x 5 block never above it by more than 1e-2 relative,
and the goal has a potential exactly when the reference found one.

Every case of the fixture runs here: the library's API expresses them all."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_planner_reference_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

PLANS, META = T.load()
BY_NAME = {p.name: p for p in PLANS}


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mirrored(p, axis):
    """the map flipped along axis (0: y, 1: x) and the end points in the mirrored cells, sub-cell offsets kept"""
    n = p.cmap.shape[axis]

    def flip(xy):
        out = [float(xy[0]), float(xy[1])]
        v = out[1 - axis]
        out[1 - axis] = (n - 1 - int(v)) + (v - int(v))
        return out
    return np.ascontiguousarray(np.flip(p.cmap, axis=axis)), flip(p.start), flip(p.goal)


def _handle(nav, p):
    ny, nx = p.cmap.shape
    trio = [_mirrored(p, 0), (p.cmap, list(p.start), list(p.goal)), _mirrored(p, 1)]
    nf = nav.NavFn(nx, ny, 3)
    nf.set_costmap(np.stack([t[0] for t in trio]), cost_mode=0)
    starts, goals = np.array([t[1] for t in trio]), np.array([t[2] for t in trio])
    return nf, starts, goals, goals.astype(np.int32)


@pytest.mark.parametrize("name", [p.name for p in PLANS])
def test_plan_matches_the_reference(nav, name):
    p = BY_NAME[name]
    nf, starts, goals, cells = _handle(nav, p)
    assert tuple(cells[1]) == tuple(p.goal_cell)
    res = nf.global_planner_plan(starts, goals, cells, **p.params)
    got, path = nf.potential(1), nf.path(1)
    nf.close()
    d = bits(got) != bits(p.potential)
    if d.any():
        j, i = np.argwhere(d)[0]
        pytest.fail(f"{d.sum()} potentials differ, first at ({i}, {j}): {got[j, i]!r} != {p.potential[j, i]!r} (cost {p.seen[j, i]})")
    want = p.path if p.path_ret == 1 else np.zeros((0, 2), np.float32)
    assert bool(res[1].found) == (p.path_ret == 1) and res[1].path_length == len(want) == len(path)
    diff = np.nonzero((bits(path) != bits(want)).any(axis=1))[0]
    assert diff.size == 0, f"first differing point {diff[0]}: {path[diff[0]]} != {want[diff[0]]}"


@pytest.mark.parametrize("name", [p.name for p in PLANS if p.params["use_dijkstra"]])
def test_wavefront_stays_within_its_contract_of_the_reference(nav, name):
    p = BY_NAME[name]
    nf, starts, goals, cells = _handle(nav, p)
    nf.global_planner_plan(starts, goals, cells, wavefront=True, **p.params)
    g = nf.potential(1)
    nf.close()
    assert (g[p.goal_cell[1], p.goal_cell[0]] < 1e9) == bool(p.found_legal)
    m = (p.potential < 1e9) & ~p.goal_block
    over = m & (g > p.potential * np.float32(1 + 1e-2))
    assert not over.any(), f"{over.sum()} cells above the reference-order array, worst {float((g[m] / p.potential[m]).max())}"
