"""navgpu_global_planner_make_plan / _plans / _potential_grid on the GPU against tests/global_plan_ref.py (the reference's lines
restated, pinned on the CPU by tests/test_global_plan_reference.py) applied to what the CPU oracle's global_planner core returns.

Positions must be equal as float64 bits.  Yaws must agree within 1e-12 rad: every input of the yaw arithmetic is bit-equal, the
one operation that may differ is atan2 (device libm against glibc: a few units in the last place of a value <= pi, about 1e-15);
interpolation multiplies an increment error of that size divided by (b - a) by an index <= b.  Each test prints the largest
difference it saw."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_plan_ref as R  # noqa: E402
from test_navfn import GP_VARIANTS  # noqa: E402

pytestmark = pytest.mark.gpu
YAW_TOL = 1e-12
MODES = [R.NONE, R.FORWARD, R.INTERPOLATE, R.FORWARD_THEN_INTERPOLATE]
NAVGPU_ERR_STATE = -5


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    return nav


@pytest.fixture(scope="module")
def core(orc):
    """the oracle's expansion + traceback, each distinct plan computed once for all the tests of this file"""
    inner, seen = R.oracle_core(orc), {}

    def cached(cm, s, g, gc, **kw):
        key = (cm.shape, cm.tobytes(), tuple(s), tuple(g), tuple(gc), tuple(sorted(kw.items())))
        if key not in seen:
            path, pot = inner(cm, s, g, gc, **kw)
            path.setflags(write=False)
            pot.setflags(write=False)
            seen[key] = (path, pot)
        return seen[key]
    return cached


@pytest.fixture(scope="module")
def handles(nav):
    made = {}

    def get(nx, ny, n):
        if (nx, ny, n) not in made:
            made[(nx, ny, n)] = nav.NavFn(nx, ny, n)
        return made[(nx, ny, n)]
    yield get
    for nf in made.values():
        nf.close()


def _load(nf, cases):
    nf.set_costmap(np.stack([c[0] for c in cases]), cost_mode=0)
    return (np.array([c[1] for c in cases]), np.array([c[2] for c in cases], np.float64), np.array([c[3] for c in cases], np.float64))


def _compare(res, poses, offsets, refs, what):
    """statuses, counts and offsets equal; x, y bit-equal; yaw within YAW_TOL.  -> the largest yaw difference"""
    worst = 0.0
    assert offsets[0] == 0
    for k, ref in enumerate(refs):
        assert res[k].status == ref["status"], (what, k, res[k].status, ref["status"])
        assert res[k].n_poses == ref["n_poses"], (what, k, res[k].n_poses, ref["n_poses"])
        assert int(offsets[k + 1]) - int(offsets[k]) == ref["n_poses"], (what, k)
        if ref["start_cell"] is not None and ref["goal_cell"] is not None:
            assert tuple(res[k].start_cell) == tuple(ref["start_cell"]) and tuple(res[k].goal_cell) == tuple(ref["goal_cell"]), (what, k)
        assert bool(res[k].found) == (ref["n_poses"] > 0), (what, k)
        got = poses[offsets[k]:offsets[k + 1]]
        want = ref["poses"]
        assert np.array_equal(got[:, :2].view(np.uint64), np.ascontiguousarray(want[:, :2]).view(np.uint64)), f"{what}: plan {k}: positions differ"
        if len(want):
            d = float(np.abs(got[:, 2] - want[:, 2]).max())
            worst = max(worst, d)
            assert d <= YAW_TOL, f"{what}: plan {k}: yaw differs by {d:.3e}"
    assert int(offsets[-1]) == sum(r["n_poses"] for r in refs) == len(poses)
    print(f"{what}: largest yaw difference {worst:.3e} rad")
    return worst


def _run(nf, core, cases, mode, kw, what):
    frames, starts, goals = _load(nf, cases)
    res = nf.make_plan(frames, starts, goals, orientation_mode=mode, **kw)
    poses, offsets = nf.plans(0, len(cases))
    refs = [R.make_plan(core, *c, mode, **kw) for c in cases]
    _compare(res, poses, offsets, refs, what)
    return res, refs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", GP_VARIANTS)
def test_make_plan_matches_the_restatement(handles, core, kw, mode):
    """Six plans of 11 - 62 poses, and between them one each that starts off the map, ends off the map, is walled off and starts
    inside the border limit: each carries its own status and the neighbours are what they are without it."""
    cases, statuses = R.batch_cases()
    res, refs = _run(handles(48, 48, len(cases)), core, cases, mode, kw, f"batch {kw} mode {mode}")
    for k, st in enumerate(statuses):
        if st != R.OK:
            assert res[k].status == st, (k, res[k].status, st)
    assert sum(r["n_poses"] > 0 for r in refs) >= 1


@pytest.mark.parametrize("mode", MODES[1:])
@pytest.mark.parametrize("kw", [dict(), dict(use_grid_path=1)])
def test_long_plans(handles, core, kw, mode):
    """The serpentine's plans take more than two chunks of a workgroup (> 512 poses with the gradient path)."""
    cases = R.serpentine_cases()
    res, refs = _run(handles(64, 64, len(cases)), core, cases, mode, kw, f"serpentine {kw} mode {mode}")
    assert all(r.n_poses > (256 if kw else 512) for r in res)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", [dict(), dict(use_grid_path=1), dict(old_navfn_behavior=1)])
def test_short_plans(handles, core, kw, mode):
    cases = R.short_cases()
    res, refs = _run(handles(48, 48, len(cases)), core, cases, mode, kw, f"short {kw} mode {mode}")
    counts = {r.n_poses for r in res}
    assert counts & {2, 3, 4}, counts


@pytest.mark.parametrize("mode", [R.NONE, R.FORWARD_THEN_INTERPOLATE])
@pytest.mark.parametrize("kw", [dict(), dict(use_quadratic=0, old_navfn_behavior=1)])
def test_wavefront(handles, kw, mode):
    """wavefront = 1: the restatement applied to the device's own navgpu_navfn_path / navgpu_navfn_potential of that call (the
    wavefront's path is not the oracle's, by its existing contract)."""
    cases, statuses = R.batch_cases()
    nf = handles(48, 48, len(cases))
    frames, starts, goals = _load(nf, cases)
    res = nf.make_plan(frames, starts, goals, orientation_mode=mode, wavefront=True, **kw)
    poses, offsets = nf.plans(0, len(cases))
    refs = [R.make_plan(lambda *a, _k=k, **b: (nf.path(_k), nf.potential(_k)), *c, mode, **kw) for k, c in enumerate(cases)]
    _compare(res, poses, offsets, refs, f"wavefront {kw} mode {mode}")
    assert [r.status for r in res] == statuses
    grids, maxima = nf.potential_grid(0, len(cases))
    for k, ref in enumerate(refs):
        if ref["potential"] is not None:
            g, mx = R.potential_grid(ref["potential"], 100)
            assert np.array_equal(grids[k], g) and np.float32(maxima[k]).view(np.uint32) == np.float32(mx).view(np.uint32), k


def test_clear_robot_cell(nav, handles, core):
    """A lethal start cell still gives a plan; the cost array shows FREE_SPACE there afterwards; path and potential are those of
    navgpu_global_planner_plan on the map with that cell cleared by hand."""
    cm, frame, start, goal = R.random_cases()[0]
    st, sc, gc, s, g = R.endpoints(frame, start, goal, 48, 48)
    assert st == R.OK
    blocked = cm.copy()
    blocked[sc[1], sc[0]] = 254
    nf = handles(48, 48, 2)
    nf.set_costmap(np.stack([blocked, blocked]), cost_mode=0)
    assert nf.costarr(0)[sc[1], sc[0]] == 254
    res = nf.make_plan(frame, [start], [goal], first=0, orientation_mode=R.FORWARD)
    assert res[0].status == R.OK and res[0].n_poses > 2
    assert nf.costarr(0)[sc[1], sc[0]] == 0 and nf.costarr(1)[sc[1], sc[0]] == 254
    path, pot = nf.path(0), nf.potential(0)
    by_hand = blocked.copy()
    by_hand[sc[1], sc[0]] = 0
    nf.set_costmap(by_hand[None], first=1, count=1, cost_mode=0)
    r1 = nf.global_planner_plan([s], [g], [gc], first=1)
    assert r1[0].found and r1[0].path_length == res[0].n_poses - 1
    assert np.array_equal(nf.path(1).view(np.uint32), path.view(np.uint32))
    assert np.array_equal(nf.potential(1).view(np.uint32), pot.view(np.uint32))
    ref = R.make_plan(core, blocked, frame, start, goal, R.FORWARD)
    assert ref["n_poses"] == res[0].n_poses


def test_buffer_conventions(nav, core):
    import ctypes as C
    cases, _ = R.batch_cases()
    n = len(cases)
    nf = nav.NavFn(48, 48, n)
    L = nf.L
    offsets = np.zeros(n + 1, np.uint32)
    assert L.navgpu_global_planner_plans(nf.h, 0, n, 0, None, offsets.ctypes.data_as(C.c_void_p)) == NAVGPU_ERR_STATE  # nothing made yet
    frames, starts, goals = _load(nf, cases)
    assert L.navgpu_global_planner_plans(nf.h, 0, n, 0, None, offsets.ctypes.data_as(C.c_void_p)) == NAVGPU_ERR_STATE
    res = nf.make_plan(frames, starts, goals, orientation_mode=R.FORWARD_THEN_INTERPOLATE)
    true_offsets = np.concatenate([[0], np.cumsum([r.n_poses for r in res])]).astype(np.uint32)
    total = int(true_offsets[-1])
    # counts only
    assert L.navgpu_global_planner_plans(nf.h, 0, n, 0, None, offsets.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(offsets, true_offsets)
    # everything, twice: identical bytes
    a, oa = nf.plans(0, n)
    b, ob = nf.plans(0, n)
    assert len(a) == total and a.tobytes() == b.tobytes() and oa.tobytes() == ob.tobytes()
    # a capacity inside the third plan with poses: nothing at or behind it is written, what is before it is the plan's
    cap = int(true_offsets[3]) + 5
    assert 0 < cap < total
    guard = np.full((total + 8, 3), -7.25)
    offsets[:] = 0
    assert L.navgpu_global_planner_plans(nf.h, 0, n, cap, guard.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(offsets, true_offsets)
    assert (guard[cap:] == -7.25).all()
    assert guard[:cap].tobytes() == a[:cap].tobytes()
    # a sub-range
    c, oc = nf.plans(2, 3)
    assert c.tobytes() == a[true_offsets[2]:true_offsets[5]].tobytes() and np.array_equal(oc, true_offsets[2:6] - true_offsets[2])
    # new costs for one plan: the range that holds it has no plans any more, the others keep theirs
    nf.set_costmap(cases[2][0][None], first=2, count=1, cost_mode=0)
    assert L.navgpu_global_planner_plans(nf.h, 0, n, 0, None, offsets.ctypes.data_as(C.c_void_p)) == NAVGPU_ERR_STATE
    d, od = nf.plans(3, n - 3)
    assert d.tobytes() == a[true_offsets[3]:].tobytes()
    nf.close()


@pytest.mark.parametrize("kw", [dict(), dict(use_dijkstra=0, use_quadratic=0, use_grid_path=1)])
def test_potential_grid(handles, core, kw):
    """Equal to the restatement on the oracle's potential array, the walled-off plan (nothing found) included; maxima as float bits."""
    cases, statuses = R.batch_cases()
    res, refs = _run(handles(48, 48, len(cases)), core, cases, R.NONE, kw, f"grid {kw}")
    nf = handles(48, 48, len(cases))
    for scale in (100, 127):
        grids, maxima = nf.potential_grid(0, len(cases), publish_scale=scale)
        for k, ref in enumerate(refs):
            if ref["potential"] is None:
                continue
            g, mx = R.potential_grid(ref["potential"], scale)
            assert np.float32(maxima[k]).view(np.uint32) == np.float32(mx).view(np.uint32), (k, maxima[k], mx)
            assert np.array_equal(grids[k], g), f"plan {k} scale {scale}: {np.count_nonzero(grids[k] != g)} cells differ"
    assert refs[statuses.index(R.NO_PLAN)]["potential"] is not None


def test_potential_grid_odd_size(nav, handles, core):
    """67 x 45 = 3015 cells: no multiple of the workgroup, rows no multiple of a wave."""
    from test_navfn import _random_costmap
    rs = np.random.RandomState(5)
    nx, ny = 67, 45
    frame = (-0.4, 0.9, 0.05)
    cases = []
    for _ in range(2):
        cm = _random_costmap(rs, 80, 0.03)[:ny, :nx].copy()
        s, g = (rs.uniform(6, 14), rs.uniform(6, ny - 8)), (rs.uniform(nx - 16, nx - 8), rs.uniform(6, ny - 8))
        for x, y in (s, g):
            cm[int(y) - 1:int(y) + 3, int(x) - 1:int(x) + 3] = 0
        cases.append((cm, frame, R.world_pose(frame, s, 0.5), R.world_pose(frame, g, -1.0)))
    nf = handles(nx, ny, 2)
    res, refs = _run(nf, core, cases, R.FORWARD, dict(), "odd size")
    assert all(r.status == R.OK for r in res)
    fresh = nav.NavFn(nx, ny, 1)  # nothing planned: every potential is 0, the maximum is 0 and the library writes 0
    g0, m0 = fresh.potential_grid()
    assert not g0.any() and m0[0] == 0
    fresh.close()
    grids, maxima = nf.potential_grid(publish_scale=100)
    for k, ref in enumerate(refs):
        g, mx = R.potential_grid(ref["potential"], 100)
        assert np.float32(maxima[k]).view(np.uint32) == np.float32(mx).view(np.uint32)
        assert np.array_equal(grids[k], g)
        assert (g == -1).any() and (g >= 0).any()
