"""navgpu_navfn_ros_* on the GPU against tests/navfn_ros_ref.py (the reference's lines restated, pinned on the CPU by
tests/test_navfn_ros_reference.py) applied to what the CPU oracle's NavFn returns.

Everything is compared bit for bit: cells, counts and statuses as integers, costs and poses as float64 bits, potentials and cloud
points as float32 bits.  Each operation is the same IEEE operation on both sides (fp64 +, -, *, /, sqrt; fp32 /, *), correctly
rounded on both, without contraction: no tolerance is due."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navfn_ros_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAVGPU_ERR_INVALID, NAVGPU_ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    return nav


@pytest.fixture(scope="module")
def ref(orc):
    """the yardstick's make_plan, each distinct plan computed once for all the tests of this file and left unchanged"""
    seen = {}

    def cached(cm, frame, start, goal, tol, w_dist=1.0, w_len=0.0):
        key = (cm.shape, cm.tobytes(), tuple(frame), tuple(start), tuple(goal), float(tol), float(w_dist), float(w_len))
        if key not in seen:
            seen[key] = R.make_plan(orc, cm, frame, start, goal, tol, w_dist, w_len)
            for v in seen[key].values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
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


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _args(cases):
    return (np.array([c[1] for c in cases]), np.array([c[2] for c in cases], np.float64), np.array([c[3] for c in cases], np.float64),
            np.array([c[4] for c in cases], np.float64))


def _check_plan(nf, k, res, poses, want, what, potential=True):
    assert res.status == want["status"], (what, k, res.status, want["status"])
    assert res.n_poses == want["n_poses"] == len(poses), (what, k, res.n_poses, want["n_poses"], len(poses))
    if want["start_cell"] is not None:
        assert tuple(res.start_cell) == tuple(want["start_cell"]), (what, k)
    if want["goal_cell"] is None:
        return
    assert tuple(res.goal_cell) == tuple(want["goal_cell"]), (what, k)
    assert res.candidates == want["candidates"], (what, k, res.candidates, want["candidates"])
    b = want["best"]
    if b is None:
        assert tuple(res.best_cell) == (-1, -1), (what, k)
    else:
        assert tuple(res.best_cell) == tuple(b["cell"]), (what, k, tuple(res.best_cell), b["cell"])
        assert np.array_equal(_bits64([res.best_x, res.best_y, res.best_cost]), _bits64([b["x"], b["y"], b["cost"]])), (what, k)
    if potential:
        assert bool(res.found) == want["found"] and res.cycles == want["cycles"], (what, k, res.found, res.cycles, want["found"], want["cycles"])
        assert np.array_equal(_bits32(nf.potential(k)), _bits32(want["potential"])), f"{what}: plan {k}: potential differs"
    if want["status"] == R.OK:
        assert np.array_equal(_bits32(nf.path(k)), _bits32(want["path"])), f"{what}: plan {k}: path differs"
    else:
        assert len(nf.path(k)) == 0, f"{what}: plan {k}: a path is handed out for a plan that has none"
    assert np.array_equal(_bits64(poses), _bits64(want["poses"])), f"{what}: plan {k}: poses differ"


def test_batch_matches_the_restatement(handles, ref):
    """Twelve plans on one handle: six random ones with tolerances 0 - 0.25 m, and between them a start off the map, a goal off the map
    with tolerance 0 and with 0.3 (cell (0, 0)), a goal inside a lethal blob with tolerance 0.3 (best pose != goal) and 0, a walled-off
    goal and a negative tolerance."""
    cases, statuses = R.batch_cases()
    nf = handles(48, 48, len(cases))
    nf.set_costmap(np.stack([c[0] for c in cases]), cost_mode=1)
    frames, starts, goals, tols = _args(cases)
    res = nf.navfn_ros_make_plan(frames, starts, goals, tols)
    poses, offsets = nf.navfn_ros_plans(0, len(cases))
    assert offsets[0] == 0 and int(offsets[-1]) == len(poses)
    wants = [ref(*c) for c in cases]
    for k, (want, st) in enumerate(zip(wants, statuses)):
        assert want["status"] == st and res[k].status == st, (k, res[k].status, want["status"], st)
        _check_plan(nf, k, res[k], poses[offsets[k]:offsets[k + 1]], want, "batch")
    blocked = wants[6]
    assert blocked["best"]["cell"] != blocked["goal_cell"] and blocked["poses"][-1, 2] == cases[6][3][2]
    assert wants[5]["goal_cell"] == (0, 0) and wants[5]["n_poses"] > 0
    assert sum(w["n_poses"] > 0 for w in wants) >= 7
    # a second read gives the same bytes; a short capacity keeps the offsets true and writes no further
    poses2, offsets2 = nf.navfn_ros_plans(0, len(cases))
    assert poses2.tobytes() == poses.tobytes() and offsets2.tobytes() == offsets.tobytes()
    short, offsets3 = nf.navfn_ros_plans(0, len(cases), capacity=30)
    assert offsets3.tobytes() == offsets.tobytes() and short.tobytes() == poses[:30].tobytes()


@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.0, 1.0), (1.0, 0.01)])
def test_weights_choose_the_cell(handles, ref, weights):
    """The blocked goal under three weightings, and the obstacle-free ring whose nearest candidates tie exactly under (1, 0)."""
    cm, frame, s, g = R.blocked_goal_case()
    rcm, rframe, rs, rg, rtol = R.ring_case()
    nf = handles(48, 48, 2)
    nf.set_costmap(np.stack([cm, rcm]), cost_mode=1)
    res = nf.navfn_ros_make_plan([frame, rframe], [s, rs], [g, rg], [0.3, rtol], w_dist=weights[0], w_len=weights[1])
    poses, offsets = nf.navfn_ros_plans(0, 2)
    wants = [ref(cm, frame, s, g, 0.3, *weights), ref(rcm, rframe, rs, rg, rtol, *weights)]
    for k in range(2):
        _check_plan(nf, k, res[k], poses[offsets[k]:offsets[k + 1]], wants[k], f"weights {weights}")
    picks = {w: ref(cm, frame, s, g, 0.3, *w)["best"]["cell"] for w in [(1.0, 0.0), (0.0, 1.0)]}
    assert picks[(1.0, 0.0)] != picks[(0.0, 1.0)]
    if weights == (1.0, 0.0):  # four candidates 3 cells from the goal tie; the first in scan order is the one below it
        gc = wants[1]["goal_cell"]
        pot = wants[1]["potential"]
        ring = [(gc[0], gc[1] - 3), (gc[0] - 3, gc[1]), (gc[0] + 3, gc[1]), (gc[0], gc[1] + 3)]
        assert all(pot[c[1], c[0]] < R.POT_HIGH for c in ring)
        assert tuple(res[1].best_cell) == ring[0] and res[1].best_cost == 3 * rframe[2]


def test_path_longer_than_the_limit_is_no_plan(handles, ref, orc):
    """64 x 64 serpentine: the goal has a potential and the expansion's own calcPath(nx * ny / 2) finds a path, but
    getPlanFromPotential's calcPath(nx * 4) runs out of steps: an empty plan."""
    cm, frame, s, g = R.serpentine_case()
    want = ref(cm, frame, s, g, 0.0)
    unlimited = orc.navfn_calc_path(want["potential"], want["start_cell"], want["goal_cell"])
    assert len(unlimited) > 4 * 64 and want["found"] and want["candidates"] == 1 and want["status"] == R.NO_PLAN
    nf = handles(64, 64, 1)
    nf.set_costmap(cm, cost_mode=1)
    res = nf.navfn_ros_make_plan(frame, [s], [g], 0.0)
    poses, offsets = nf.navfn_ros_plans(0, 1)
    _check_plan(nf, 0, res[0], poses, want, "serpentine")
    assert res[0].found == 1 and res[0].status == R.NO_PLAN and res[0].n_poses == 0 and list(offsets) == [0, 0] and len(nf.path(0)) == 0


def test_wavefront_option(handles, orc):
    """The tiled wavefront's own potential array, read back, under the yardstick's window and calcPath; the array against the update
    rule's fixed point at and below the start's potential (navgpu_navfn_plan_wavefront's contract); two runs give the same bytes."""
    cases = [c + (t,) for c, t in zip(R.random_cases()[:3], (0.0, 0.2, 0.1))] + [R.blocked_goal_case() + (0.3,)]
    nf = handles(48, 48, len(cases))
    nf.set_costmap(np.stack([c[0] for c in cases]), cost_mode=1)
    frames, starts, goals, tols = _args(cases)
    runs = []
    for _ in range(2):
        res = nf.navfn_ros_make_plan(frames, starts, goals, tols, wavefront=True)
        poses, offsets = nf.navfn_ros_plans(0, len(cases))
        pots = [nf.potential(k) for k in range(len(cases))]
        runs.append((bytes(b"".join(bytes(r) for r in res)), poses.tobytes(), offsets.tobytes(), b"".join(p.tobytes() for p in pots)))
    assert runs[0] == runs[1]
    for k, c in enumerate(cases):
        want = R.make_plan(orc, *c, potential=pots[k])
        _check_plan(nf, k, res[k], poses[offsets[k]:offsets[k + 1]], want, "wavefront", potential=False)
        assert want["status"] == R.OK
        _, fixed = orc.navfn_fixed_point(c[0], want["start_cell"], want["goal_cell"], cost_mode=1)
        gc = want["goal_cell"]
        if fixed[gc[1], gc[0]] < R.POT_HIGH:
            low = fixed <= fixed[gc[1], gc[0]]
            assert np.array_equal(_bits32(pots[k][low]), _bits32(fixed[low])), k


def test_potential_queries_after_compute_potential(handles, orc):
    """computePotential of two points (and one off the map), then getPlanFromPotential, getPointPotential over a 7 x 7 grid that
    hangs off the map, and validPointPotential with tolerances 0 and 0.2 next to a pocket nothing reaches."""
    cm, frame = R.pocket_case()
    ox, oy, res_ = frame
    nf = handles(48, 48, 3)
    nf.set_costmap(cm, cost_mode=1)
    points = [R.cell_pose(frame, (10, 12), 0)[:2], R.cell_pose(frame, (30, 8), 0)[:2], [ox - 1.0, oy + 1.0]]
    res = nf.navfn_ros_compute_potential(frame, points)
    wants = [R.compute_potential(orc, cm, frame, p) for p in points]
    assert [r.status for r in res] == [R.OK, R.OK, R.GOAL_OFF_MAP]
    for k in range(2):
        cell, pot, found = wants[k]
        assert tuple(res[k].goal_cell) == cell and bool(res[k].found) == found
        assert np.array_equal(_bits32(nf.potential(k)), _bits32(pot)), k
    # getPointPotential: a 7 x 7 grid from 0.4 m left of / below the map to its far side
    grid = np.array([[ox - 0.4 + i * 0.45, oy - 0.4 + j * 0.45] for j in range(7) for i in range(7)])
    got = nf.navfn_ros_point_potential(frame, [grid, grid[::-1], grid[:0]])
    want = [R.point_potential(wants[0][1], frame, x, y) for x, y in grid] + [R.point_potential(wants[1][1], frame, x, y) for x, y in grid[::-1]]
    assert np.array_equal(_bits64(got), _bits64(want))
    assert (np.array(want) == R.DBL_MAX).sum() >= 13 * 2 and (np.array(want) < R.POT_HIGH).sum() >= 20
    # validPointPotential: the pocket's centre (5 cells from its wall), beside its wall inside, in the open and off the map
    pts = np.array([R.cell_pose(frame, (36, 36), 0)[:2], R.cell_pose(frame, (32, 36), 0)[:2], R.cell_pose(frame, (20, 20), 0)[:2], [ox - 0.1, oy + 1.0]])
    q = [np.concatenate([pts, pts]), pts, pts[:0]]
    tol = np.array([0.0] * 4 + [0.2] * 4 + [0.2] * 4)
    flags = nf.navfn_ros_valid_point_potential(frame, q, tol)
    want = [R.valid_point_potential(wants[0][1], frame, p, t) for p, t in zip(q[0], tol[:8])] + \
           [R.valid_point_potential(wants[1][1], frame, p, t) for p, t in zip(q[1], tol[8:])]
    assert list(flags) == [int(v) for v in want]
    assert list(flags[:8]) == [0, 0, 1, 0, 0, 1, 1, 1]
    # getPlanFromPotential to the computePotential point of each plan: from the open, from the pocket, from off the map
    goals = [R.cell_pose(frame, (40, 20), 0.3), R.cell_pose(frame, (36, 36), 0.1), [ox - 1.0, oy, 0.0]]
    pr = nf.navfn_ros_plan_from_potential(frame, goals)
    poses, offsets = nf.navfn_ros_plans(0, 3)
    robot = [wants[0][0], wants[1][0], (0, 0)]
    pots = [wants[0][1], wants[1][1], wants[1][1]]
    for k in range(3):
        want = R.plan_from_potential(orc, pots[k], frame, goals[k], robot[k])
        assert pr[k].status == want["status"] and pr[k].n_poses == want["n_poses"], (k, pr[k].status, want["status"])
        assert np.array_equal(_bits64(poses[offsets[k]:offsets[k + 1]]), _bits64(want["poses"])), k
        if want["status"] == R.OK:
            assert np.array_equal(_bits32(nf.path(k)), _bits32(want["path"])), k
    assert [r.status for r in pr] == [R.OK, R.NO_PLAN, R.GOAL_OFF_MAP] and pr[0].n_poses > 10 and (poses[:, 2] == 0).all()


def _cloud_equal(got, want):
    return got.shape == want.shape and np.array_equal(_bits32(got), _bits32(want))  # (NaNs of one operation have one bit pattern)


def test_potential_cloud(handles, ref, orc):
    """After a found plan (divisor: the best cell's potential), a not-found one (divisor POT_HIGH), one whose start is the goal's cell
    (divisor 0: inf and NaN); count-only, short-capacity and two-plan calls."""
    rnd = R.random_cases()
    cm0, fr0, s0, g0 = rnd[0]
    blocked = R.blocked_goal_case()
    cases = [rnd[1] + (0.1,), blocked + (0.0,), (cm0, fr0, s0, s0, 0.0)]
    nf = handles(48, 48, len(cases))
    nf.set_costmap(np.stack([c[0] for c in cases]), cost_mode=1)
    frames, starts, goals, tols = _args(cases)
    res = nf.navfn_ros_make_plan(frames, starts, goals, tols)
    wants = [ref(*c) for c in cases]
    assert [r.status for r in res] == [R.OK, R.NO_PLAN, R.OK]
    clouds = [R.potential_cloud(w["potential"], c[1], w["nav_start"]) for w, c in zip(wants, cases)]
    assert wants[1]["potential"][wants[1]["nav_start"][1], wants[1]["nav_start"][0]] >= R.POT_HIGH
    assert wants[2]["nav_start"] == wants[2]["start_cell"] and np.isnan(clouds[2][:, 2]).sum() == 1 and np.isinf(clouds[2][:, 2]).sum() >= 1
    pts, offsets = nf.navfn_ros_potential_cloud(frames)
    assert list(offsets) == list(np.cumsum([0] + [len(c) for c in clouds]))
    for k, c in enumerate(clouds):
        assert _cloud_equal(pts[offsets[k]:offsets[k + 1]], c), k
    # count only; a capacity that ends inside plan 1; a two-plan range that does not begin at plan 0
    _, only = nf.navfn_ros_potential_cloud(frames, capacity=0)
    assert only.tobytes() == offsets.tobytes()
    cap = int(offsets[1]) + 17
    short, off2 = nf.navfn_ros_potential_cloud(frames, capacity=cap)
    assert off2.tobytes() == offsets.tobytes() and short.tobytes() == pts[:cap].tobytes()
    two, off3 = nf.navfn_ros_potential_cloud(frames[1:], first=1, count=2)
    assert list(off3) == [0, len(clouds[1]), len(clouds[1]) + len(clouds[2])] and two.tobytes() == pts[offsets[1]:].tobytes()
    # after compute_potential NavFn's start is (0, 0): an unreached border cell
    nf.navfn_ros_compute_potential(frames[0], [starts[0][:2]], first=0)
    _, pot, _ = R.compute_potential(orc, cases[0][0], cases[0][1], starts[0][:2])
    one, _ = nf.navfn_ros_potential_cloud(frames[:1], first=0, count=1)
    assert _cloud_equal(one, R.potential_cloud(pot, cases[0][1], (0, 0)))


def test_state(handles, nav, ref):
    """Whatever else writes a plan's costs or path takes navfn_ros_plans away for that plan; the two make_plan families do not read
    each other's; a sub-range call leaves the other plans alone; an over-long window is refused before anything runs."""
    cases = [c + (0.1,) for c in R.random_cases()] + [R.blocked_goal_case() + (0.3,), R.blocked_goal_case() + (0.0,)]
    nf = handles(48, 48, len(cases))
    n = len(cases)
    L = nf.L
    off = np.zeros(n + 1, np.uint32)

    def ros_plans_rc(first, count):
        return L.navgpu_navfn_ros_plans(nf.h, first, count, 0, None, off.ctypes.data)

    def gp_plans_rc(first, count):
        return L.navgpu_global_planner_plans(nf.h, first, count, 0, None, off.ctypes.data)

    nf.set_costmap(np.stack([c[0] for c in cases]), cost_mode=1)
    frames, starts, goals, tols = _args(cases)
    assert ros_plans_rc(0, n) == NAVGPU_ERR_STATE
    res = nf.navfn_ros_make_plan(frames, starts, goals, tols)
    poses, offsets = nf.navfn_ros_plans(0, n)
    assert gp_plans_rc(0, n) == NAVGPU_ERR_STATE
    # a sub-range call with other tolerances: plans 3 .. 6 change, the others keep results, poses and potentials
    before = [nf.potential(k) for k in range(n)]
    sub = nf.navfn_ros_make_plan(frames[3:7], starts[3:7], goals[3:7], [0.0, 0.2, 0.3, 0.2], first=3)
    poses2, offsets2 = nf.navfn_ros_plans(0, n)
    for k in range(n):
        if 3 <= k < 7:
            want = ref(*cases[k][:4], [0.0, 0.2, 0.3, 0.2][k - 3])
            _check_plan(nf, k, sub[k - 3], poses2[offsets2[k]:offsets2[k + 1]], want, "sub-range")
        else:
            assert poses2[offsets2[k]:offsets2[k + 1]].tobytes() == poses[offsets[k]:offsets[k + 1]].tobytes(), k
            assert nf.potential(k).tobytes() == before[k].tobytes(), k
    # set_costmap and navgpu_navfn_plan on single plans
    nf.set_costmap(cases[1][0], first=1, count=1, cost_mode=1)
    nf.plan([ref(*cases[4])["start_cell"]], [ref(*cases[4])["goal_cell"]], first=4)
    assert ros_plans_rc(1, 1) == NAVGPU_ERR_STATE and ros_plans_rc(4, 1) == NAVGPU_ERR_STATE and ros_plans_rc(0, n) == NAVGPU_ERR_STATE
    assert ros_plans_rc(0, 1) == 0 and ros_plans_rc(2, 2) == 0 and ros_plans_rc(5, n - 5) == 0
    # global_planner's make_plan on plan 2 (its costs are read as the costmap itself there; only the state matters here)
    nf.make_plan(frames[2:3], starts[2:3], goals[2:3], first=2)
    assert ros_plans_rc(2, 1) == NAVGPU_ERR_STATE and gp_plans_rc(2, 1) == 0 and gp_plans_rc(3, 1) == NAVGPU_ERR_STATE
    # the window limit: 4097 candidates per axis
    res_ = frames[0][2]
    big = np.array([4096.5 * res_ / 2] * 1)
    pr = nav._lib.NavfnRosParams(1.0, 0.0, 0, 0)
    out = (nav._lib.NavfnRosResult * 1)()
    fr0, st0, gl0 = (np.ascontiguousarray(a[:1]) for a in (frames, starts, goals))
    rc = L.navgpu_navfn_ros_make_plan(nf.h, 0, 1, pr, fr0.ctypes.data, st0.ctypes.data, gl0.ctypes.data, big.ctypes.data, out)
    assert rc == NAVGPU_ERR_INVALID
    assert ros_plans_rc(0, 1) == 0  # nothing ran: plan 0 is still the first call's
    ok = np.array([4094.5 * res_ / 2])
    assert L.navgpu_navfn_ros_make_plan(nf.h, 0, 1, pr, fr0.ctypes.data, st0.ctypes.data, gl0.ctypes.data, ok.ctypes.data, out) == 0


def test_costs_from_a_fleet(nav, ref):
    """Costs handed over on the device from a 2-robot fleet's master grids give what the same bytes uploaded from the host give."""
    from navigation_amd import _lib as N, synth
    cases = [c + (0.1,) for c in R.random_cases()[:2]]
    fl = nav.Fleet(2, 48, 48, R.RES, layers=N.LAYER_OBSTACLE | N.LAYER_INFLATION)
    fl.configure_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, synth.inscribed_radius(synth.FOOTPRINT))
    fl.upload(N.GRID_MASTER, np.stack([c[0] for c in cases]))
    masters = fl.master()
    assert all(np.array_equal(masters[k], cases[k][0]) for k in range(2))
    frames, starts, goals, tols = _args(cases)
    a, b = nav.NavFn(48, 48, 2), nav.NavFn(48, 48, 2)
    try:
        a.set_costmap_from_fleet(fl, allow_unknown=True)
        b.set_costmap(np.stack([c[0] for c in cases]), cost_mode=1, allow_unknown=True)
        ra = a.navfn_ros_make_plan(frames, starts, goals, tols)
        rb = b.navfn_ros_make_plan(frames, starts, goals, tols)
        pa, oa = a.navfn_ros_plans()
        pb, ob = b.navfn_ros_plans()
        assert b"".join(bytes(r) for r in ra) == b"".join(bytes(r) for r in rb)
        assert pa.tobytes() == pb.tobytes() and oa.tobytes() == ob.tobytes() and len(pa) > 0
        for k in range(2):
            assert a.potential(k).tobytes() == b.potential(k).tobytes()
            _check_plan(a, k, ra[k], pa[oa[k]:oa[k + 1]], ref(*cases[k]), "fleet")
    finally:
        a.close()
        b.close()
        fl.close()
