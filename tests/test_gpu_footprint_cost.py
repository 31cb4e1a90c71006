"""navgpu_footprint_cost, navgpu_rotate_recovery_* and navgpu_carrot_plan through the C-ABI against the CPU oracle's
CostmapModel::footprintCost (oracle.pyoracle.footprint_cost) and restatements, written here, of
RotateRecovery::runBehavior (rotate_recovery/src/rotate_recovery.cpp:100-153) and CarrotPlanner::makePlan
(carrot_planner/src/carrot_planner.cpp:116-169).  Expected doubles are compared with ==.

Condition on the inputs: the device's cos / sin may differ from the host's in the last bit, so every test asserts on the host
that no oriented vertex of any query lies within 1e-9 cell of a cell boundary (_assert_off_boundaries); seeds and poses are
chosen so that no query has to be left out.  Need a real MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LETHAL, INSCRIBED, NOINFO = 254, 253, 255
RES = 0.05
FP2 = [[0.1, 0.0], [-0.1, 0.0]]                                   # "circular" robot: < 3 vertices
TRI = [[0.18, 0.0], [-0.12, 0.13], [-0.1, -0.15]]
RECT = [[0.2, 0.15], [-0.2, 0.15], [-0.2, -0.15], [0.2, -0.15]]
PENT = [[0.19, 0.01], [0.07, 0.17], [-0.16, 0.1], [-0.15, -0.11], [0.05, -0.18]]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


@pytest.fixture(scope="module")
def N():
    from navigation_amd import _lib
    return _lib


def _norm(a):  # angles::normalize_angle, the fmod form of navgpu_shortest_angular_distance
    r = math.fmod(math.fmod(a, 2.0 * math.pi) + 2.0 * math.pi, 2.0 * math.pi)
    if r > math.pi:
        r -= 2.0 * math.pi
    return r


def _assert_off_boundaries(poses, fp, ox, oy, res=RES):
    """no oriented vertex within 1e-9 cell of a cell boundary (robots with < 3 vertices read the centre cell only: no trig)"""
    p = np.asarray(poses, np.float64).reshape(-1, 3)
    fp = np.asarray(fp, np.float64).reshape(-1, 2)
    if len(fp) < 3 or len(p) == 0:
        return
    c, s = np.cos(p[:, 2:3]), np.sin(p[:, 2:3])
    wx = p[:, 0:1] + (fp[:, 0] * c - fp[:, 1] * s)
    wy = p[:, 1:2] + (fp[:, 0] * s + fp[:, 1] * c)
    for w, o in ((wx, ox), (wy, oy)):
        f = (w - o) / res
        assert np.abs(f - np.rint(f)).min() > 1e-9, "a vertex lies on a cell boundary: choose another pose / seed"


def _expected(orc, grid, ox, oy, poses, fp, allow_unknown):
    return np.array([orc.footprint_cost(grid, RES, ox, oy, x, y, th, fp, bool(allow_unknown)) for x, y, th in poses], np.float64)


def _first_illegal(costs):
    bad = np.nonzero(costs < 0)[0]
    return int(bad[0]) if len(bad) else -1


def _fp16(N):
    xy = np.zeros((16, 2))
    assert N.lib().navgpu_footprint_from_radius(0.2, xy.ctypes.data_as(C.c_void_p)) == 0
    return xy.tolist()


# ----------------------------------------------------------------------------------------------
# the primitive: 5 robots with different footprints on a 60 x 60 map with a non-zero origin
# ----------------------------------------------------------------------------------------------
OX, OY = -1.0, 0.5


def _prim_grid():
    g = np.zeros((60, 60), np.uint8)
    yy, xx = np.mgrid[10:20, 30:40]
    g[10:20, 30:40] = (1 + (xx * 7 + yy * 13) % 252).astype(np.uint8)  # inflated values 1..252
    g[22:26, 8:30] = 97
    g[40:50, 5:15] = INSCRIBED
    g[30, 30] = LETHAL                                                # one lethal cell on its own
    g[50:55, 40:50] = LETHAL
    g[5:12, 45:55] = NOINFO
    return g


def _cell_centre(cx, cy, ox=OX, oy=OY):
    return ox + (cx + 0.5) * RES, oy + (cy + 0.5) * RES


def _explicit_poses(fp):
    v0 = fp[0]
    lx, ly = _cell_centre(30, 30)
    return [
        (OX + 1.731, OY + 0.742, -2.2),                   # 0: over the inflated values
        (OX + 10 * RES + 0.012, OY + 45 * RES + 0.013, 0.0),  # 1: outline inside the INSCRIBED patch: legal for polygons only
        (OX + 50 * RES + 0.012, OY + 8 * RES + 0.013, 0.4),   # 2: in the NO_INFORMATION patch
        (lx - v0[0], ly - v0[1], 0.0),                    # 3: vertex 0 in the lone LETHAL cell, nothing else of the outline near it
        (OX + 0.112, OY + 1.513, 0.1),                    # 4: centre on the map, a vertex off it (every polygon reaches > 0.112 m)
        (OX - 0.3, OY + 1.0, 0.3),                        # 5: centre off the map
    ]


def _runs(fps, counts, seed):
    rs = np.random.RandomState(seed)
    runs = []
    for fp, n in zip(fps, counts):
        p = _explicit_poses(fp)[:n]
        while len(p) < n:
            p.append((rs.uniform(OX - 0.05, OX + 3.05), rs.uniform(OY - 0.05, OY + 3.05), rs.uniform(-math.pi, math.pi)))
        runs.append(np.array(p, np.float64).reshape(-1, 3))
    return runs


@pytest.fixture(scope="module")
def prim(nav, N):
    fps = [FP2, TRI, RECT, PENT, _fp16(N)]
    grid = _prim_grid()
    fl = nav.Fleet(5, 60, 60, RES, layers=N.LAYER_OBSTACLE)
    fl.set_origin([[OX, OY]] * 5)
    for k, fp in enumerate(fps):
        fl.set_footprint(fp, first=k, count=1)
    fl.upload(N.GRID_MASTER, np.stack([grid] * 5))
    yield dict(fl=fl, fps=fps, grid=grid)
    fl.close()


# run lengths 0, 1, 63, 65, 200 cross wave and workgroup boundaries and leave one run empty; the second assignment gives the
# 16-gon (16 queries per workgroup) the long runs
@pytest.mark.parametrize("allow_unknown", [0, 1])
@pytest.mark.parametrize("counts", [(65, 63, 200, 1, 0), (1, 0, 63, 65, 200)])
def test_footprint_cost_equals_oracle(prim, orc, counts, allow_unknown):
    fl, fps, grid = prim["fl"], prim["fps"], prim["grid"]
    fl.set_origin([[OX, OY]] * 5)
    runs = _runs(fps, counts, seed=11 + counts[0])
    for fp, p in zip(fps, runs):
        _assert_off_boundaries(p, fp, OX, OY)
    costs, first_illegal = fl.footprint_cost(runs, allow_unknown=allow_unknown)
    for k, (fp, p) in enumerate(zip(fps, runs)):
        want = _expected(orc, grid, OX, OY, p, fp, allow_unknown)
        print(f"robot {k}: {len(p)} queries, {int((want < 0).sum())} illegal, first illegal {_first_illegal(want)}")
        assert np.array_equal(costs[k], want), (k, np.nonzero(costs[k] != want)[0][:8])
        assert first_illegal[k] == _first_illegal(want), (k, first_illegal[k])
        # the hand-made cases are what they claim to be
        n = len(p)
        if n > 0:
            assert 0.0 < want[0] < 253.0
        if n > 1:
            assert want[1] == (-1.0 if len(fp) < 3 else float(INSCRIBED))
        if n > 2:
            assert want[2] == (float(NOINFO) if allow_unknown else -1.0)
        if n > 5:
            assert want[5] == -1.0
            if len(fp) >= 3:
                assert want[3] == -1.0 and want[4] == -1.0
                q = p[3].copy()
                q[:2] += 2 * RES  # the same outline two cells further on misses the lone lethal cell
                assert orc.footprint_cost(grid, RES, OX, OY, *q, fp, bool(allow_unknown)) >= 0
    # the window moves (Costmap2D::updateOrigin's effect on the geometry): the same world poses, the oracle's new answers
    ox2, oy2 = OX + 0.37, OY - 0.21
    fl.set_origin([[ox2, oy2]] * 5)
    for fp, p in zip(fps, runs):
        _assert_off_boundaries(p, fp, ox2, oy2)
    costs, first_illegal = fl.footprint_cost(runs, allow_unknown=allow_unknown)
    moved = 0
    for k, (fp, p) in enumerate(zip(fps, runs)):
        want = _expected(orc, grid, ox2, oy2, p, fp, allow_unknown)
        moved += int((want != _expected(orc, grid, OX, OY, p, fp, allow_unknown)).sum())
        assert np.array_equal(costs[k], want), (k, np.nonzero(costs[k] != want)[0][:8])
        assert first_illegal[k] == _first_illegal(want)
    assert moved > 0  # (the move changes answers: the test would notice a stale origin)
    fl.set_origin([[OX, OY]] * 5)


def test_footprint_cost_tiny_footprint_and_long_edges(nav, N, orc):
    """a footprint smaller than a cell (every vertex in one cell) and edges longer than 64 cells, on a 200 x 40 map"""
    tiny = [[0.004, 0.0], [-0.003, 0.004], [-0.002, -0.005]]
    plank = [[2.0, 0.1], [-2.0, 0.1], [-2.0, -0.1], [2.0, -0.1]]  # 80-cell edges
    ox, oy = 3.0, -1.0
    grid = np.zeros((40, 200), np.uint8)
    grid[18:22, 60:64] = 180
    grid[30, 100] = LETHAL
    grid[5:8, 150:160] = INSCRIBED
    fl = nav.Fleet(2, 200, 40, RES, layers=N.LAYER_OBSTACLE)
    fl.set_origin([[ox, oy]] * 2)
    fl.set_footprint(tiny, first=0, count=1)
    fl.set_footprint(plank, first=1, count=1)
    fl.upload(N.GRID_MASTER, np.stack([grid] * 2))
    cx, cy = ox + 100.5 * RES, oy + 30.5 * RES
    rs = np.random.RandomState(3)
    p_tiny = [(ox + 61.5 * RES, oy + 19.5 * RES, 0.7), (cx, cy, 0.0), (ox + 10.5 * RES, oy + 10.5 * RES, 2.0), (ox + 155.5 * RES, oy + 6.5 * RES, -1.0)]
    p_tiny += [(rs.uniform(ox, ox + 10), rs.uniform(oy, oy + 2), rs.uniform(-3, 3)) for _ in range(30)]
    p_plank = [(ox + 5.012, oy + 1.013, 0.0), (ox + 5.012, oy + 1.013, 0.05), (ox + 5.012, oy + 1.013, -0.1), (ox + 5.012, oy + 1.013, math.pi),
               (ox + 5.012, oy + 1.413, 0.02),   # the long edge runs through the lethal cell's row
               (ox + 1.012, oy + 1.013, 0.0)]    # an end off the map
    p_plank += [(rs.uniform(ox + 2.1, ox + 7.9), rs.uniform(oy + 0.5, oy + 1.5), rs.uniform(-0.2, 0.2)) for _ in range(40)]
    runs = [np.array(p_tiny), np.array(p_plank)]
    for fp, p in zip((tiny, plank), runs):
        _assert_off_boundaries(p, fp, ox, oy)
    costs, first_illegal = fl.footprint_cost(runs, allow_unknown=False)
    for k, (fp, p) in enumerate(zip((tiny, plank), runs)):
        want = _expected(orc, grid, ox, oy, p, fp, False)
        print(f"robot {k}: {len(p)} queries, {int((want < 0).sum())} illegal, largest cost {want.max()}")
        assert np.array_equal(costs[k], want), (k, np.nonzero(costs[k] != want)[0][:8])
        assert first_illegal[k] == _first_illegal(want)
    want_tiny = _expected(orc, grid, ox, oy, runs[0], tiny, False)
    assert list(want_tiny[:4]) == [180.0, -1.0, 0.0, float(INSCRIBED)]
    assert (_expected(orc, grid, ox, oy, runs[1], plank, False)[:4] >= 0).all()
    fl.close()


# ----------------------------------------------------------------------------------------------
# ordering: a query queued behind a costmap update sees what the update wrote, with no sync in between
# ----------------------------------------------------------------------------------------------
def test_footprint_cost_is_ordered_behind_costmap_update(nav, N, orc):
    fl = nav.Fleet(1, 60, 60, RES, layers=N.LAYER_OBSTACLE, max_points=16)
    fl.configure_obstacle()
    fl.set_footprint(RECT)
    pose = np.array([[1.512, 1.513, 0.0]])
    _assert_off_boundaries(pose, RECT, 0.0, 0.0)
    costs, fi = fl.footprint_cost([pose], allow_unknown=False)
    assert costs[0][0] == 0.0 and fi[0] == -1
    # one marking point in the cell of vertex 0; the costmap's own robot stands far away (its footprint is cleared there)
    px, py = 1.512 + 0.2, 1.513 + 0.15
    pts = np.array([[px, py, 0.5]], np.float32)
    fl.stage_observations([[0.4, 0.4, 0.0]], [dict(instance=0, points=pts, origin=(0.4, 0.4, 1.0), obstacle_range=100.0, raytrace_range=100.0)])
    fl.update_map()  # queued, not waited for
    costs, fi = fl.footprint_cost([pose], allow_unknown=False)
    master = fl.master()[0]
    assert master[int(py / RES), int(px / RES)] == LETHAL
    assert costs[0][0] == -1.0 and fi[0] == 0
    assert costs[0][0] == orc.footprint_cost(master, RES, 0.0, 0.0, *pose[0], RECT, False)
    fl.close()


# ----------------------------------------------------------------------------------------------
# rotate recovery
# ----------------------------------------------------------------------------------------------
NOSE = [[0.4, 0.1], [-0.1, 0.1], [-0.1, -0.1], [0.4, -0.1]]  # reaches 0.41 m ahead, 0.14 m behind: no rotational symmetry


def _rotate_ref(orc, grid, fp, P, pose, st):
    """one pass of the while(n.ok()) body, rotate_recovery.cpp:105-153 (with :100-104 on the first pass of a run)"""
    x, y, yaw = pose
    if not st["started"]:
        st.update(start_offset=0 - _norm(yaw), got_180=0, started=1)
    current_angle = _norm(_norm(yaw) + st["start_offset"])
    dist_left = math.pi - current_angle
    sim_angle, n, thetas = 0.0, 0, []
    while sim_angle < dist_left:
        theta = yaw + sim_angle
        thetas.append(theta)
        n += 1
        if orc.footprint_cost(grid, RES, 0.0, 0.0, x, y, theta, fp, bool(P.allow_unknown)) < 0.0:
            st.update(started=0, swept=n)
            return 0.0, 2, thetas
        sim_angle += P.sim_granularity
    st["swept"] = n
    vel = math.sqrt(2 * P.acc_lim_th * dist_left)
    vel = min(max(vel, P.min_in_place_rotational_vel), P.max_rotational_vel)
    if current_angle < 0.0:
        st["got_180"] = 1
    if st["got_180"] and current_angle >= (0.0 - P.yaw_goal_tolerance):
        st["started"] = 0
        return vel, 1, thetas
    return vel, 0, thetas


def test_rotate_recovery_steps_equal_restatement(nav, N, orc):
    n = 80
    grid = np.zeros((n, n), np.uint8)
    grid[8:14, 8:14] = 120
    # robot 2 faces a lethal cell: nose edge at x = 3.012 + 0.4
    grid[int(1.013 / RES), int((3.012 + 0.4) / RES)] = LETHAL
    # robot 3: a lethal cell 0.35 m from the centre at 170 degrees from its start heading - out of reach of the tail (0.14 m),
    # met by the nose after some 150 degrees of the sweep
    c3 = (3.012, 3.013, 0.2)
    grid[int((c3[1] + 0.35 * math.sin(c3[2] + math.radians(170))) / RES), int((c3[0] + 0.35 * math.cos(c3[2] + math.radians(170))) / RES)] = LETHAL
    poses = np.array([(1.012, 1.013, 0.3), (1.012, 3.013, 3.1), (3.012, 1.013, 0.0), c3], np.float64)
    fl = nav.Fleet(4, n, n, RES, layers=N.LAYER_OBSTACLE)
    fl.set_footprint(NOSE)
    fl.upload(N.GRID_MASTER, np.stack([grid] * 4))
    P = N.RotateRecoveryParams()  # the reference's defaults
    fl.configure_rotate_recovery(P)
    states = (N.RotateRecoveryState * 4)()
    ref = [dict(start_offset=0.0, got_180=0, started=0, swept=0) for _ in range(4)]
    done_at, seen = [None] * 4, [set() for _ in range(4)]
    for step in range(400):
        wz, status = fl.rotate_recovery_step(poses, states)
        for k in range(4):
            want_wz, want_status, thetas = _rotate_ref(orc, grid, NOSE, P, poses[k], ref[k])
            _assert_off_boundaries([(poses[k][0], poses[k][1], t) for t in thetas], NOSE, 0.0, 0.0)
            got = (wz[k], int(status[k]), states[k].start_offset, states[k].got_180, states[k].started, states[k].swept)
            want = (want_wz, want_status, ref[k]["start_offset"], ref[k]["got_180"], ref[k]["started"], ref[k]["swept"])
            assert got == want, (step, k, got, want)
            seen[k].add(want_status)
            if want_status == 1 and done_at[k] is None:
                done_at[k] = step
            if step == 0:
                print(f"robot {k}: first step status {want_status}, swept {ref[k]['swept']}, cmd_wz {want_wz}")
        if done_at[0] is not None and done_at[1] is not None:
            break
        poses[:, 2] += wz / 20.0  # (blocked robots get 0)
        poses[1, 2] = _norm(poses[1, 2])  # robot 1 reports its yaw the way getYaw does, wrapped at +-pi
    print("done at steps", done_at)
    assert done_at[0] is not None and done_at[1] is not None and min(done_at[0], done_at[1]) > 100  # a full turn at <= 1 rad/s, 20 Hz
    assert seen[0] == {0, 1} and seen[1] == {0, 1}
    assert seen[2] == {2} and seen[3] == {2}
    assert ref[2]["swept"] == 1 and 100 < ref[3]["swept"] < 185  # blocked at the first heading / near the end of the sweep
    fl.close()


# ----------------------------------------------------------------------------------------------
# carrot planner
# ----------------------------------------------------------------------------------------------
def _carrot_ref(orc, grid, fp, start, goal, allow_unknown):
    """carrot_planner.cpp:116-169; returns (target, done, candidates tried, candidates)"""
    start_x, start_y, start_yaw = start
    goal_x, goal_y, goal_yaw = goal
    diff_x, diff_y = goal_x - start_x, goal_y - start_y
    diff_yaw = _norm(goal_yaw - start_yaw)
    target = (goal_x, goal_y, goal_yaw)
    done, scale, d_scale, tried, cands = False, 1.0, 0.01, 0, []
    while not done:
        if scale < 0:
            target = (start_x, start_y, start_yaw)
            break
        target = (start_x + scale * diff_x, start_y + scale * diff_y, _norm(start_yaw + scale * diff_yaw))
        cands.append(target)
        tried += 1
        if len(fp) >= 3 and orc.footprint_cost(grid, RES, 0.0, 0.0, *target, fp, bool(allow_unknown)) >= 0:
            done = True
        scale -= d_scale
    return target, done, tried, cands


def test_carrot_plan_equals_restatement(nav, N, orc):
    n = 80
    grid = np.zeros((n, n), np.uint8)
    grid[30:50, 50:70] = LETHAL      # a block: x 2.5 .. 3.5, y 1.5 .. 2.5
    grid[60:64, 10:30] = 200
    plans = [
        ((0.512, 0.513, 0.1), (2.012, 0.713, 0.5)),      # goal legal
        ((0.712, 2.013, 0.0), (3.012, 2.113, 1.0)),      # goal inside the block, a legal point partway
        ((2.912, 1.913, 0.3), (3.112, 2.113, -0.4)),     # start and goal inside the block: nothing legal
        ((1.512, 3.213, -0.7), (1.512, 3.213, -0.7)),    # start = goal
        ((0.712, 1.813, 3.0), (3.012, 2.013, -3.0)),     # the yaw difference crosses +-pi, goal inside the block
        ((1.012, 3.413, 0.2), (1.912, 4.713, 0.9)),      # goal off the map
    ]
    fl = nav.Fleet(len(plans), n, n, RES, layers=N.LAYER_OBSTACLE)
    fl.set_footprint(RECT)
    fl.upload(N.GRID_MASTER, np.stack([grid] * len(plans)))
    starts = np.array([p[0] for p in plans])
    goals = np.array([p[1] for p in plans])
    targets, found = fl.carrot_plan(starts, goals, allow_unknown=False)
    dones = []
    for k, (s, g) in enumerate(plans):
        want, done, tried, cands = _carrot_ref(orc, grid, RECT, s, g, False)
        _assert_off_boundaries(cands, RECT, 0.0, 0.0)
        print(f"plan {k}: done {done}, tried {tried}, target {want}")
        assert tuple(targets[k]) == want, (k, tuple(targets[k]), want)
        assert found[k] == (tried if done else 0), (k, found[k], tried, done)
        dones.append((done, tried))
    assert dones[0] == (True, 1) and dones[3] == (True, 1)
    assert dones[1][0] and dones[1][1] > 1 and dones[4][0] and dones[4][1] > 1 and dones[5][0] and dones[5][1] > 1
    assert not dones[2][0] and dones[2][1] >= 100 and tuple(targets[2]) == plans[2][0]
    # CarrotPlanner::footprintCost refuses a footprint of fewer than 3 vertices (:76-79)
    fl.set_footprint(FP2, first=0, count=1)
    targets, found = fl.carrot_plan(starts[:1], goals[:1], allow_unknown=False)
    assert found[0] == 0 and tuple(targets[0]) == plans[0][0]
    fl.close()


# ----------------------------------------------------------------------------------------------
# errors: the project's codes, and nothing changes
# ----------------------------------------------------------------------------------------------
def test_errors_leave_state_untouched(nav, N):
    L = N.lib()
    fl = nav.Fleet(2, 60, 60, RES, layers=N.LAYER_OBSTACLE)
    fl.set_footprint(RECT)
    h = fl.h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    counts = np.array([1, 1], np.uint32)
    poses = np.array([[1.012, 1.013, 0.1], [1.512, 1.013, 0.2]])
    costs = np.full(2, 7.0)
    fi = np.full(2, 7, np.int32)
    st = (N.RotateRecoveryState * 2)()
    wz = np.full(2, 7.0)
    status = np.full(2, 7, np.int32)
    targets = np.full((2, 3), 7.0)
    found = np.full(2, 7, np.int32)
    INVALID, CAPACITY = -1, -4
    # null pointers
    assert L.navgpu_footprint_cost(None, 0, 2, vp(counts), vp(poses), 0, vp(costs), vp(fi)) == INVALID
    assert L.navgpu_footprint_cost(h, 0, 2, None, vp(poses), 0, vp(costs), vp(fi)) == INVALID
    assert L.navgpu_footprint_cost(h, 0, 2, vp(counts), None, 0, vp(costs), vp(fi)) == INVALID
    assert L.navgpu_footprint_cost(h, 0, 2, vp(counts), vp(poses), 0, None, vp(fi)) == INVALID
    assert L.navgpu_rotate_recovery_configure(h, None) == INVALID
    assert L.navgpu_rotate_recovery_step(h, 0, 2, vp(poses), None, vp(wz), vp(status)) == INVALID
    assert L.navgpu_rotate_recovery_step(h, 0, 2, None, C.cast(st, C.c_void_p), vp(wz), vp(status)) == INVALID
    assert L.navgpu_carrot_plan(h, 0, 2, vp(poses), vp(poses), 0, None, vp(found)) == INVALID
    assert L.navgpu_carrot_plan(h, 0, 2, vp(poses), None, 0, vp(targets), vp(found)) == INVALID
    # a pose that is not finite
    for bad in (float("nan"), float("inf")):
        q = poses.copy()
        q[1, 2] = bad
        assert L.navgpu_footprint_cost(h, 0, 2, vp(counts), vp(q), 0, vp(costs), vp(fi)) == INVALID
        assert L.navgpu_rotate_recovery_step(h, 0, 2, vp(q), C.cast(st, C.c_void_p), vp(wz), vp(status)) == INVALID
        assert L.navgpu_carrot_plan(h, 0, 2, vp(poses), vp(q), 0, vp(targets), vp(found)) == INVALID
    # ranges past the fleet
    assert L.navgpu_footprint_cost(h, 1, 2, vp(counts), vp(poses), 0, vp(costs), vp(fi)) == INVALID
    assert L.navgpu_footprint_cost(h, 2, 1, vp(counts), vp(poses), 0, vp(costs), vp(fi)) == INVALID
    assert L.navgpu_rotate_recovery_step(h, 1, 2, vp(poses), C.cast(st, C.c_void_p), vp(wz), vp(status)) == INVALID
    assert L.navgpu_carrot_plan(h, 0, 3, vp(poses), vp(poses), 0, vp(targets), vp(found)) == INVALID
    assert (costs == 7.0).all() and (fi == 7).all() and (wz == 7.0).all() and (status == 7).all() and (targets == 7.0).all() and (found == 7).all()
    assert all(s.started == 0 and s.swept == 0 and s.start_offset == 0.0 for s in st)
    # a sim_granularity whose sweep would exceed the capacity, or none at all: refused, the configuration in force stays
    fl.configure_rotate_recovery(sim_granularity=0.05)
    for bad, code in ((2.0 * math.pi / 5000, CAPACITY), (0.0, INVALID), (-0.017, INVALID), (float("nan"), INVALID)):
        p = N.RotateRecoveryParams(sim_granularity=bad, max_rotational_vel=9.0)
        assert L.navgpu_rotate_recovery_configure(h, C.byref(p)) == code, bad
    wz, status = fl.rotate_recovery_step(poses, st)
    assert [s.swept for s in st] == [63, 63]  # ceil(pi / 0.05): still the 0.05 sweep
    assert (wz == 1.0).all() and (status == 0).all()  # ... and the 1.0 rad/s limit
    fl.close()
