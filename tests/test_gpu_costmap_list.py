"""The costmap update for a robot list (navgpu_costmap_stage_list / navgpu_obsbuf_stage_list / navgpu_costmap_update_list /
navgpu_costmap_bounds_list).  Need a real MI355X.

Nothing in the update reduces across robots, so the bar is bit equality throughout.
  1. fixed window: a fleet driven through the listed calls against a twin driven through the range calls, contiguous run by contiguous
     run; and, for the robots outside the list, the fleet against itself before the listed calls;
  2. rolling window, which the range calls take for the whole fleet only: twelve oracles, of which only the listed ones get a cycle -
     all twelve robots against their oracle after every cycle; and the planner's view of a listed-updated rolling fleet against one-robot
     rolling twins driven through the range calls;
  3. errors; 4. the launches of a listed update, counted.
Shapes (tests/test_costmap_list_abi.py asserts what they select): twelve robots, 80 rows, width 96 (k_merge's 16-aligned form) and 130
(the unaligned form, three 64 x 32 inflation tiles in each direction), scans of at most 720 points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_costmap_list_abi import INFLATION, N_ROBOTS, NINE, RES, ROWS, WIDTH_ALIGNED, WIDTH_UNALIGNED  # noqa: E402

pytestmark = pytest.mark.gpu

NAVGPU_OK, NAVGPU_ERR_INVALID, NAVGPU_ERR_CAPACITY, NAVGPU_ERR_STATE = 0, -1, -4, -5
LETHAL = 254
FULL, SINGLE, THREE = tuple(range(N_ROBOTS)), (4,), (1, 6, 11)
COMPLEMENT = tuple(i for i in range(N_ROBOTS) if i not in NINE)
OBS_RANGE, RAY_RANGE = 2.5, 3.0
# fixed-window variants: the layer's form, the sensors, footprint clearing, the inflation kernel, the static layer's merge
VARIANTS = {
    "2d": dict(nx=WIDTH_UNALIGNED),
    "2d_aligned": dict(nx=WIDTH_ALIGNED),
    "voxel": dict(nx=WIDTH_UNALIGNED, voxel=True),
    "voxel_aligned_marks_ordered": dict(nx=WIDTH_ALIGNED, voxel=True, mark_threshold=1),
    "two_sensors": dict(nx=WIDTH_ALIGNED, two_sensors=True),
    "voxel_two_sensors": dict(nx=WIDTH_UNALIGNED, voxel=True, two_sensors=True),
    "no_footprint_clearing": dict(nx=WIDTH_ALIGNED, footprint_clearing=False),
    "inflate_bits_generic": dict(nx=WIDTH_UNALIGNED, inflation="bits"),
    "inflate_tile": dict(nx=WIDTH_UNALIGNED, inflation="tile"),
    "inflate_priority_queue": dict(nx=WIDTH_ALIGNED, pq=True),
    "static_use_maximum": dict(nx=WIDTH_ALIGNED, static="max"),
    "static_overwrite": dict(nx=WIDTH_UNALIGNED, static="overwrite"),
    "two_cycles_in_flight": dict(nx=WIDTH_ALIGNED, in_flight=2),  # the mirrors and the block wait for the marker behind their copy
}


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _runs(robots):
    """the contiguous runs (first, count) of a strictly increasing list"""
    runs = []
    for r in robots:
        if runs and runs[-1][0] + runs[-1][1] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    return [tuple(r) for r in runs]


_WORLD = {}


def _world():
    from navigation_amd import synth
    if "w" not in _WORLD:
        w = synth.make_instance(400, 41)  # 20 m x 20 m of scattered lethal cells, two walls, three moving discs
        w["cells"].setflags(write=False)
        _WORLD["w"] = w
    return _WORLD["w"]


_SCANS = {}


def _scan(x, y, yaw, cyc, voxel):
    """a 720-beam scan of the world from a pose; computed once per pose and left unchanged"""
    from navigation_amd import synth
    key = (round(float(x), 6), round(float(y), 6), round(float(yaw), 6), cyc, voxel)
    if key not in _SCANS:
        inst = dict(_world())
        inst["pos"] = np.array([x, y, yaw], np.float32)
        pts = synth.laser_scan(inst, cyc, max_range=4.0, z=0.3, z_jitter=1.2 if voxel else None)
        assert 0 < len(pts) <= 720
        pts.setflags(write=False)
        _SCANS[key] = pts
    return _SCANS[key]


def _observations(i, pose, cyc, v):
    """robot i's observations of a cycle: one marking + clearing sensor, or a marking-only and a clearing-only one"""
    pts = _scan(pose[0], pose[1], pose[2], cyc, bool(v.get("voxel")))
    org = (float(pose[0]), float(pose[1]), 0.3)
    if not v.get("two_sensors"):
        return [dict(instance=i, points=pts, origin=org, obstacle_range=OBS_RANGE, raytrace_range=RAY_RANGE)]
    return [dict(instance=i, points=pts, origin=org, obstacle_range=OBS_RANGE, raytrace_range=RAY_RANGE, marking=True, clearing=False),
            dict(instance=i, points=pts[::2].copy(), origin=org, obstacle_range=OBS_RANGE, raytrace_range=RAY_RANGE, marking=False, clearing=True)]


def _fleet(nav, v, n=N_ROBOTS, rolling=False, planner=False, track_unknown=False):
    from navigation_amd import _lib as N, synth
    nx = v["nx"]
    voxel = bool(v.get("voxel"))
    layers = (N.LAYER_VOXEL if voxel else N.LAYER_OBSTACLE) | N.LAYER_INFLATION | (N.LAYER_STATIC if v.get("static") or v.get("rolling_static") else 0)
    fl = nav.Fleet(n, nx, ROWS, RES, layers=layers, track_unknown=track_unknown, max_points=1440, max_observations=2, rolling_window=rolling,
                   max_sim_steps=32, max_plan=64)
    fl.configure_obstacle(footprint_clearing_enabled=v.get("footprint_clearing", True), mark_threshold=v.get("mark_threshold", 0))
    fl.set_footprint(synth.FOOTPRINT)
    fl.configure_inflation(INFLATION[v.get("inflation", "bits11")], synth.COST_SCALING, synth.inscribed_radius(synth.FOOTPRINT),
                           priority_queue_order=bool(v.get("pq")))
    if v.get("static"):
        fl.add_static_map(_static_occ(nx), use_maximum=v["static"] == "max")
    if v.get("in_flight"):
        fl.set_cycles_in_flight(v["in_flight"])
    if planner:
        fl.configure_planner(nav.DwaConfig(vx_samples=5, vy_samples=1, vth_samples=7, sim_time=1.0, sim_granularity=0.1, discretize_by_time=1))
    return fl


def _static_occ(nx):
    rs = np.random.RandomState(5)
    occ = np.where(_world()["cells"][:ROWS, :nx] == LETHAL, 100, 0).astype(np.int8)
    occ[rs.random_sample(occ.shape) < 0.02] = -1
    occ[10, 5:40] = 100
    return occ


def _fixed_pose(nx, i, cyc):
    """robot i's pose in cycle cyc on a fixed window: near the middle of the map, moving a little every cycle"""
    rs = np.random.RandomState(300 + i)
    x, y = nx * RES / 2 + rs.uniform(-0.5, 0.5), ROWS * RES / 2 + rs.uniform(-0.4, 0.4)
    return [float(x + 0.06 * cyc), float(y - 0.04 * cyc), float(0.5 * i + 0.3 * cyc)]


def _snapshot(fl, voxel, with_status):
    from navigation_amd import _lib as N
    s = dict(master=fl.master(), layer=fl.download(N.GRID_OBSTACLE), box=fl.bounds())
    if voxel:
        s["voxels"] = fl.download(N.GRID_VOXEL)
    if with_status:
        s["obs_status"] = np.array([np.frombuffer(bytes(st), np.uint8) for st in fl.obs_status()])
    return s


def _twin_cycles(nav, variant, robots):
    """fleet A through the listed calls, fleet B through the range calls run by run; returns nothing, asserts everything"""
    from navigation_amd import _lib as N
    v = VARIANTS[variant]
    nx, voxel = v["nx"], bool(v.get("voxel"))
    robots = list(robots)
    others = [i for i in range(N_ROBOTS) if i not in robots]
    A, B = _fleet(nav, v), _fleet(nav, v)
    try:
        flags = [N.OBS_MARKING, N.OBS_CLEARING] if v.get("two_sensors") else [N.OBS_MARKING | N.OBS_CLEARING]
        for fl in (A, B):
            fl.obs_configure([dict(obstacle_range=OBS_RANGE, raytrace_range=RAY_RANGE, flags=f) for f in flags], slots=1, max_cloud_points=720)
            poses = [_fixed_pose(nx, i, 0) for i in range(N_ROBOTS)]  # a whole-fleet range cycle first: every robot owns state
            fl.stage_observations(poses, [o for i in range(N_ROBOTS) for o in _observations(i, poses[i], 0, v)])
            fl.update_map()
        before = _snapshot(A, voxel, True)
        for cyc in (1, 2, 3):
            poses = [_fixed_pose(nx, i, cyc) for i in robots]
            obs = {i: _observations(i, poses[k], cyc, v) for k, i in enumerate(robots)}
            if cyc != 2:  # from host observations
                A.stage_observations_list(robots, poses, [o for i in robots for o in obs[i]])
                for first, count in _runs(robots):
                    k = robots.index(first)
                    B.stage_observations(poses[k:k + count], [o for i in robots[k:k + count] for o in obs[i]], first=first)
            else:  # from the resident buffer: the scans arrive once, the stage names the robots
                now = 1000000000 * cyc
                clouds = [dict(instance=i, source=s, stamp_ns=now, origin=o["origin"], points=o["points"]) for i in robots for s, o in enumerate(obs[i])]
                for fl in (A, B):
                    fl.obs_buffer(clouds, now)
                cur_a = A.obs_stage_list(robots, poses, now)
                cur_b = np.concatenate([B.obs_stage(poses[k:k + count], now, first=first) for first, count in _runs(robots) for k in [robots.index(first)]])
                assert np.array_equal(cur_a, cur_b) and cur_a.all()
            A.update_map_list(robots)
            for first, count in _runs(robots):
                B.update_map(first, count)
            a, b = _snapshot(A, voxel, True), _snapshot(B, voxel, True)
            assert np.array_equal(A.bounds_list(robots), b["box"][robots]), (variant, cyc, "bounds_list")
            for what in a:
                for i in robots:
                    assert np.array_equal(a[what][i], b[what][i]), (variant, cyc, what, "robot", i)
                for i in others:  # nobody outside the list was touched
                    assert np.array_equal(a[what][i], before[what][i]), (variant, cyc, what, "unlisted robot", i)
            assert all((a["master"][i] == LETHAL).sum() > 0 for i in robots), "a listed robot marked nothing: the scene tells nothing"
            # (with a static layer of the same world the master may come out as before: the layer grid still moves with the robot)
            assert any(not np.array_equal(a[g][i], before[g][i]) for i in robots for g in ("master", "layer")), "the cycle changed nothing"
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------------------------------------ 1. fixed window, twin fleets
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_listed_update_equals_range_updates(nav, variant):
    _twin_cycles(nav, variant, NINE)


@pytest.mark.parametrize("variant", ["2d_aligned", "voxel"])
@pytest.mark.parametrize("robots", [FULL, SINGLE, THREE], ids=["full", "single", "three"])
def test_full_list_single_robot_and_three(nav, variant, robots):
    _twin_cycles(nav, variant, robots)


# ------------------------------------------------------------------------------------------------ 2. rolling window against the oracle
def _rolling_pose(i, u):
    """robot i's pose at the u-th update it takes: 0.2 - 0.35 m further every time, robot 6 far away from its third update on"""
    rs = np.random.RandomState(700 + i)
    x0, y0, heading = rs.uniform(7.0, 13.0), rs.uniform(7.0, 13.0), rs.uniform(-np.pi, np.pi)
    step = rs.uniform(0.2, 0.35)
    jump = 9.0 if (i == 6 and u >= 2) else 0.0
    return [float(x0 + step * u * np.cos(heading) + jump), float(y0 + step * u * np.sin(heading) - jump / 3), float(heading + 0.2 * u)]


ROLLING_STATIC = dict(res=0.1, ox=4.0, oy=5.0)


def _rolling_static_occ():
    rs = np.random.RandomState(11)
    occ = np.zeros((100, 120), np.int8)
    occ[rs.random_sample(occ.shape) < 0.01] = 100
    occ[40:43, 10:100] = 100
    occ[rs.random_sample(occ.shape) < 0.05] = -1
    return occ


def _rolling_oracle(orc, v, track_unknown):
    from navigation_amd import synth
    o = orc.LayeredCostmap(track_unknown)
    o.resize(v["nx"], ROWS, RES, 0, 0)
    o.set_rolling(True)
    o.set_footprint(synth.FOOTPRINT)
    if v.get("rolling_static"):
        o.add_static_rolling(_rolling_static_occ(), ROLLING_STATIC["res"], ROLLING_STATIC["ox"], ROLLING_STATIC["oy"], track_unknown_space=track_unknown)
    if v.get("voxel"):
        o.add_voxel()
    else:
        o.add_obstacle()
    o.add_inflation(INFLATION["bits11"], synth.COST_SCALING, exact=True)
    o.set_footprint(synth.FOOTPRINT)
    return o


@pytest.mark.parametrize("voxel", [False, True], ids=["2d", "voxel"])
@pytest.mark.parametrize("rolling_static", [False, True], ids=["no_static", "rolling_static"])
def test_rolling_window_listed_updates_vs_oracle(nav, orc, voxel, rolling_static):
    from navigation_amd import _lib as N
    track_unknown = rolling_static
    v = dict(nx=WIDTH_UNALIGNED, voxel=voxel, rolling_static=rolling_static)
    fl = _fleet(nav, v, rolling=True, track_unknown=track_unknown)
    try:
        if rolling_static:
            fl.set_rolling_static_map(_rolling_static_occ(), ROLLING_STATIC["res"], ROLLING_STATIC["ox"], ROLLING_STATIC["oy"], track_unknown_space=track_unknown)
        oracles = [_rolling_oracle(orc, v, track_unknown) for _ in range(N_ROBOTS)]
        taken = [0] * N_ROBOTS
        shifts = []
        for cyc, robots in enumerate([NINE, COMPLEMENT, SINGLE, FULL, NINE, THREE]):
            robots = list(robots)
            poses, obs = [], []
            origin_before = fl.origins()
            for i in robots:  # only the listed robots' oracles get the cycle
                p = _rolling_pose(i, taken[i])
                o = _observations(i, p, taken[i], v)[0]
                poses.append(p)
                obs.append(o)
                oracles[i].clear_observations()
                oracles[i].add_observation(o["points"], origin=o["origin"], obstacle_range=OBS_RANGE, raytrace_range=RAY_RANGE)
                oracles[i].update_map(*p)
                taken[i] += 1
            fl.stage_observations_list(robots, poses, obs)
            fl.update_map_list(robots)
            m, ol, b, org_g = fl.master(), fl.download(N.GRID_OBSTACLE), fl.bounds(), fl.origins()
            vx = fl.download(N.GRID_VOXEL) if voxel else None
            assert np.array_equal(fl.bounds_list(robots), b[robots])
            for i in range(N_ROBOTS):  # every robot, listed or not: the unlisted ones neither shifted nor lost their grids
                tag = (cyc, i, "listed" if i in robots else "unlisted")
                assert np.array_equal(org_g[i], oracles[i].origin()), ("origin",) + tag
                assert np.array_equal(b[i], oracles[i].bounds()), ("box",) + tag
                assert np.array_equal(ol[i], oracles[i].layer(2)), ("layer",) + tag
                if voxel:
                    assert np.array_equal(vx[i], oracles[i].voxels()), ("voxels",) + tag
                assert np.array_equal(m[i], oracles[i].master()), ("master",) + tag
            if cyc:
                shifts += [np.abs(np.rint((org_g[i] - origin_before[i]) / RES)).max() for i in robots if taken[i] > 1]
        assert min(shifts) >= 2 and max(shifts) > max(v["nx"], ROWS), "windows shift by several cells, and one scrolls everything out"
        assert (m == LETHAL).sum() > 50
    finally:
        fl.close()


def test_rolling_window_planner_sees_the_listed_update(nav):
    """pl.master / origins after listed rolling updates: a planner cycle of a listed and of an unlisted robot against one-robot rolling
    twin fleets that took the same updates through the range calls"""
    v = dict(nx=WIDTH_UNALIGNED)
    fl = _fleet(nav, v, rolling=True, planner=True)
    twins = {}
    try:
        history = {i: [] for i in range(N_ROBOTS)}
        for robots in (FULL, NINE, COMPLEMENT, NINE):
            robots = list(robots)
            poses = [_rolling_pose(i, len(history[i])) for i in robots]
            obs = [_observations(i, p, len(history[i]), v)[0] for i, p in zip(robots, poses)]
            for i, p, o in zip(robots, poses, obs):
                history[i].append((p, o))
            fl.stage_observations_list(robots, poses, obs)
            fl.update_map_list(robots)
        listed, unlisted = NINE[3], COMPLEMENT[1]
        for i in (listed, unlisted):
            t = twins[i] = _fleet(nav, v, n=1, rolling=True, planner=True)
            for p, o in history[i]:
                t.stage_observations([p], [dict(o, instance=0)])
                t.update_map()
            p = history[i][-1][0]
            pos = np.array([p], np.float32)
            vel = np.array([[0.2, 0.0, 0.1]], np.float32)
            d = np.arange(0.0, 1.6, 0.05)
            plan = [np.stack([p[0] + d * np.cos(p[2]), p[1] + d * np.sin(p[2])], 1)]
            for f, first in ((fl, i), (t, 0)):
                f.set_plan()
            got = fl.find_best_path(pos, vel, plan, first=i)[0]
            want = t.find_best_path(pos, vel, plan)[0]
            assert bytes(got) == bytes(want), ("planner result", i)
            assert np.array_equal(fl.master(i, 1)[0], t.master()[0]), ("master", i)
            assert np.array_equal(fl.origins()[i], t.origins()[0]), ("origin", i)
            assert np.array_equal(fl.trajectory(i), t.trajectory(0)), ("trajectory", i)
    finally:
        fl.close()
        for t in twins.values():
            t.close()


# ------------------------------------------------------------------------------------------------ 3. errors
def _raw(fl, robots, poses, obs):
    """the arguments of navgpu_costmap_stage_list as ctypes values; returns (call, keepalive)"""
    inst = np.asarray(robots, np.uint32)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    obs_arr, pts = fl._pack_observations(obs)
    return lambda: fl.L.navgpu_costmap_stage_list(fl.h, len(inst), inst.ctypes.data, poses.ctypes.data, C.cast(obs_arr, C.c_void_p), len(obs),
                                                  pts.ctypes.data if len(pts) else None, len(pts))


def test_errors_fixed_window(nav):
    v = VARIANTS["2d_aligned"]
    nx = v["nx"]
    A, B = _fleet(nav, v), _fleet(nav, v)
    try:
        L = A.L
        A.obs_configure([dict(obstacle_range=OBS_RANGE, raytrace_range=RAY_RANGE)], slots=1, max_cloud_points=720)
        u32 = lambda a: np.asarray(a, np.uint32)  # noqa: E731
        poses = np.array([_fixed_pose(nx, i, 0) for i in range(N_ROBOTS)])
        boxes = np.zeros((N_ROBOTS + 1, 4), np.int32)
        cur = np.zeros(N_ROBOTS + 1, np.int32)

        def calls(n, ptr):
            return (L.navgpu_costmap_stage_list(A.h, n, ptr, poses.ctypes.data, None, 0, None, 0),
                    L.navgpu_obsbuf_stage_list(A.h, n, ptr, poses.ctypes.data, 0, cur.ctypes.data),
                    L.navgpu_costmap_update_list(A.h, n, ptr),
                    L.navgpu_costmap_bounds_list(A.h, n, ptr, boxes.ctypes.data))

        for bad in ([1, 1], [2, 1], [1, N_ROBOTS], list(range(N_ROBOTS)) + [N_ROBOTS]):  # duplicate, unsorted, an index >= n, too long
            arr = u32(bad)
            assert calls(len(arr), arr.ctypes.data) == (NAVGPU_ERR_INVALID,) * 4, bad
        arr = u32([0, 1])
        assert calls(0, arr.ctypes.data) == (NAVGPU_ERR_INVALID,) * 4
        assert calls(2, None) == (NAVGPU_ERR_INVALID,) * 4
        assert L.navgpu_costmap_stage_list(A.h, 2, arr.ctypes.data, None, None, 0, None, 0) == NAVGPU_ERR_INVALID
        assert L.navgpu_obsbuf_stage_list(A.h, 2, arr.ctypes.data, None, 0, None) == NAVGPU_ERR_INVALID
        assert L.navgpu_costmap_bounds_list(A.h, 2, arr.ctypes.data, None) == NAVGPU_ERR_INVALID
        assert L.navgpu_obsbuf_stage_list(B.h, 2, arr.ctypes.data, poses.ctypes.data, 0, None) == NAVGPU_ERR_STATE  # no buffer configured

        # a good stage, then stages that fail: what was staged stays, and the update runs on it
        robots = [0, 2, 3]
        good = [o for i in robots for o in _observations(i, poses[i], 0, v)]
        for fl in (A, B):
            fl.stage_observations_list(robots, poses[robots], good)
        other = _observations(1, poses[1], 0, v)
        assert _raw(A, robots, poses[robots], good + other)() == NAVGPU_ERR_INVALID      # an observation for a robot outside the list
        big = dict(good[0], points=np.zeros((1441, 3), np.float32))
        assert _raw(A, robots, poses[robots], [big])() == NAVGPU_ERR_CAPACITY             # more points than max_points
        two_halves = [dict(good[0], points=np.zeros((800, 3), np.float32))] * 2
        assert _raw(A, robots, poses[robots], two_halves)() == NAVGPU_ERR_CAPACITY        # ... in sum
        assert _raw(A, robots, poses[robots], [good[0]] * 3)() == NAVGPU_ERR_CAPACITY     # more observations than max_observations
        inst = u32(robots)
        obs_arr, pts = A._pack_observations(good)
        assert L.navgpu_costmap_stage_list(A.h, 3, inst.ctypes.data, poses.ctypes.data, C.cast(obs_arr, C.c_void_p), len(good), pts.ctypes.data,
                                           len(pts) - 1) == NAVGPU_ERR_INVALID            # points beyond the caller's array
        for fl in (A, B):
            fl.update_map_list(robots)
        assert np.array_equal(A.master(), B.master()) and (A.master()[robots] == LETHAL).sum() > 0
        assert np.array_equal(A.bounds(), B.bounds())
    finally:
        A.close()
        B.close()


def test_errors_rolling_window(nav):
    v = dict(nx=WIDTH_ALIGNED)
    fl = _fleet(nav, v, rolling=True)
    try:
        L = fl.L
        u32 = lambda a: np.asarray(a, np.uint32)  # noqa: E731

        def staged(robots, u):
            poses = [_rolling_pose(i, u) for i in robots]
            return poses, [_observations(i, p, u, v)[0] for i, p in zip(robots, poses)]

        def update(robots):
            arr = u32(robots)
            return L.navgpu_costmap_update_list(fl.h, len(arr), arr.ctypes.data)

        one = [0, 2, 3]
        poses, obs = staged(one, 0)
        fl.stage_observations_list(one, poses, obs)
        assert update([0, 2]) == NAVGPU_ERR_STATE and update([0, 2, 4]) == NAVGPU_ERR_STATE  # another set than the one staged
        assert update(list(FULL)) == NAVGPU_ERR_STATE
        assert _raw(fl, one, poses, obs)() == NAVGPU_ERR_STATE                               # a second stage before the update
        assert _raw(fl, [5], *staged([5], 0))() == NAVGPU_ERR_STATE
        assert L.navgpu_costmap_update(fl.h, 0, N_ROBOTS) == NAVGPU_ERR_STATE                # the forms do not mix
        assert update(one) == NAVGPU_OK
        before = fl.master()
        # a range stage is updated by the range call
        poses, obs = staged(list(FULL), 1)
        fl.stage_observations(poses, obs)
        assert update(list(FULL)) == NAVGPU_ERR_STATE
        fl.update_map()
        # still usable: another listed cycle moves the listed robots' windows and nobody else's
        origin_before, master_before = fl.origins(), fl.master()
        poses, obs = staged(one, 2)
        fl.stage_observations_list(one, poses, obs)
        fl.update_map_list(one)
        org, m = fl.origins(), fl.master()
        for i in range(N_ROBOTS):
            assert (i in one) != np.array_equal(org[i], origin_before[i]), i
            assert (i in one) or np.array_equal(m[i], master_before[i]), i
        assert not np.array_equal(before, m)
    finally:
        fl.close()


def test_voxel_clearing_endpoints_follow_the_listed_update(nav):
    v = VARIANTS["voxel"]
    fl = _fleet(nav, v)
    try:
        robots = [0, 2, 3]
        poses = [_fixed_pose(v["nx"], i, 0) for i in robots]
        fl.stage_observations_list(robots, poses, [_observations(i, p, 0, v)[0] for i, p in zip(robots, poses)])
        fl.update_map_list(robots)
        clouds = fl.voxel_clearing_endpoints(2, 2)  # robots 2 and 3: staged and updated through the list
        assert all(len(c[0]) > 0 for c in clouds)
        fl.stage_observations_list([2], poses[1:2], [_observations(2, poses[1], 0, v)[0]])  # staged, not updated
        counts, per_obs = np.zeros(1, np.uint32), np.zeros((1, 2), np.uint32)
        ask = lambda i: fl.L.navgpu_voxel_clearing_endpoints(fl.h, i, 1, 0, None, per_obs.ctypes.data, counts.ctypes.data)  # noqa: E731
        assert ask(2) == NAVGPU_ERR_STATE
        assert ask(3) == NAVGPU_OK and ask(0) == NAVGPU_OK
        fl.update_map_list([2])
        assert ask(2) == NAVGPU_OK
    finally:
        fl.close()


# ------------------------------------------------------------------------------------------------ 4. launch count
def test_a_listed_update_is_one_launch_of_each_kernel(nav):
    v = VARIANTS["2d"]
    fl = _fleet(nav, v)
    try:
        robots = list(NINE)
        poses = [_fixed_pose(v["nx"], i, 0) for i in robots]
        fl.stage_observations_list(robots, poses, [_observations(i, p, 0, v)[0] for i, p in zip(robots, poses)])
        fl.profile(True)
        fl.profile_reset()
        fl.update_map_list(robots)
        counts = {k: n for k, (_, n) in fl.profile_read().items()}
        fl.profile(False)
        assert (counts["k_obstacle"], counts["k_merge"], counts["k_inflate"]) == (1, 1, 1), counts
        assert sum(counts.values()) == 3, counts
    finally:
        fl.close()
