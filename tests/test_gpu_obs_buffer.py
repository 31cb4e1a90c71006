"""navgpu_obsbuf_* through the C-ABI: costmap_2d::ObservationBuffer on the device, compared with == on bytes and bits against
the restatement of tests/obs_buffer_ref.py (pinned on the CPU by tests/test_obs_buffer_host.py) evaluated with the trig that
navgpu_device_sincos returns, and - end to end - against a second fleet that takes the existing navgpu_costmap_stage path fed
the restatement's observations.  Need a real MI355X.

k_obs_ingest walks a cloud in tiles of 256 lanes (4 waves of 64) with a carry; 64 x 64 maps, 2-3 robots."""
import ctypes as C
import math

import numpy as np
import pytest

import obs_buffer_ref as R

pytestmark = pytest.mark.gpu

OK, INVALID, HIP, CAPACITY, STATE = 0, -1, -3, -4, -5
RES = 0.05
NX = NY = 64
FP = [[0.1, 0.1], [-0.1, 0.1], [-0.1, -0.1], [0.1, -0.1]]
GUARD = 12345.0
S = 1_000_000_000
F32 = np.float32


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


@pytest.fixture(scope="module")
def dev_trig(nav):
    """sin / cos exactly as the kernels evaluate them (navgpu_device_sincos)"""
    def trig(angles):
        a = np.ascontiguousarray(angles, np.float64)
        sn, cs = np.zeros_like(a), np.zeros_like(a)
        if len(a):
            assert nav.lib().navgpu_device_sincos(0, vp(a), len(a), vp(sn), vp(cs)) == OK
        return sn, cs
    return trig


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def yaw_tf(yaw, x, y, z):
    """global <- sensor: a rotation about z and a translation, as 12 doubles (basis row-major, origin)"""
    c, s = math.cos(yaw), math.sin(yaw)
    return [c, -s, 0, s, c, 0, 0, 0, 1, x, y, z]


def read_obs(fl, N, inst, now=0, slack=7):
    """navgpu_obsbuf_observations into buffers preset to GUARD, `slack` guard points behind the last -> list of dicts, and the
    guard behind the robot's last point is checked"""
    st = fl.obs_status(inst, 1)[0]
    cap_obs = max(1, fl.desc.max_observations)
    obs = (N.Observation * cap_obs)()
    pts = np.full((st.points + slack, 3), GUARD, np.float32)
    n_pts = C.c_uint32(0xDEAD)
    n = fl.L.navgpu_obsbuf_observations(fl.h, inst, now, C.cast(obs, C.c_void_p), cap_obs, vp(pts), len(pts), C.byref(n_pts))
    assert n >= 0, n
    assert n == st.kept and n_pts.value == st.points
    assert (pts[n_pts.value:] == GUARD).all(), "written behind the robot's last point"
    out, off = [], 0
    for o in obs[:n]:
        assert o.instance == inst and o.first_point == off
        out.append(dict(flags=o.flags, origin=(o.origin_x, o.origin_y, o.origin_z), obstacle_range=o.obstacle_range,
                        raytrace_range=o.raytrace_range, points=pts[off:off + o.n_points].copy()))
        off += o.n_points
    assert off == n_pts.value
    return out


def assert_same_obs(got, want, what=""):
    """counts, order, descriptors and the float bits of every point"""
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["flags"] == w["flags"] and g["obstacle_range"] == w["obstacle_range"] and g["raytrace_range"] == w["raytrace_range"], (what, k)
        assert np.array(g["origin"]).tobytes() == np.array(w["origin"], np.float64).tobytes(), (what, k, g["origin"], w["origin"])
        assert g["points"].shape == w["points"].shape, (what, k, g["points"].shape, w["points"].shape)
        assert g["points"].tobytes() == np.ascontiguousarray(w["points"], np.float32).tobytes(), (what, k)


def snapshot(fl, N):
    return [[(o["flags"], o["origin"], o["obstacle_range"], o["raytrace_range"], o["points"].tobytes()) for o in read_obs(fl, N, i)] for i in range(fl.n)]


def make_fleet(nav, N, n, layers=None, max_points=2048, max_observations=4, **kw):
    layers = (N.LAYER_OBSTACLE | N.LAYER_INFLATION) if layers is None else layers
    fl = nav.Fleet(n, NX, NY, RES, layers=layers, track_unknown=True, max_points=max_points, max_observations=max_observations, **kw)
    fl.configure_obstacle(max_obstacle_height=2.0)
    if layers & N.LAYER_INFLATION:
        fl.configure_inflation(0.3, 10.0, 0.1)
    fl.set_footprint(FP)
    return fl


# ---------------------------------------------------------------------------------------------- 1. tile and wave edges
MCP = 1024
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513, MCP)


@pytest.fixture(scope="module")
def edge_fleet(nav, N):
    fl = make_fleet(nav, N, 3)
    fl.obs_configure([dict(min_obstacle_height=0.25, max_obstacle_height=1.75)], slots=1, max_cloud_points=MCP)
    yield fl
    fl.close()


def _pattern_keep(pattern, n):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    run = int(pattern[3:])
    return (i // run) % 2 == 0


@pytest.mark.parametrize("pattern", ["all", "none", "run1", "run2", "run64"])
def test_tile_and_wave_edges(edge_fleet, N, dev_trig, pattern):
    fl = edge_fleet
    rs = np.random.RandomState(SIZES.index(513) + len(pattern))
    tf = yaw_tf(0.3, 1.1, -0.4, 0.25)  # z' = z + 0.25 in fp32
    for batch in range(0, len(SIZES), fl.n):
        sizes = SIZES[batch:batch + fl.n]
        ref = R.RefObsBuf(fl.n, [dict(min_obstacle_height=0.25, max_obstacle_height=1.75)], 1, dev_trig)
        clouds, keeps = [], []
        for r, n in enumerate(sizes):
            keep = _pattern_keep(pattern, n)
            p = rs.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
            # kept heights include both inclusive ends (z' = 0.25 and 1.75); dropped ones lie below, above, or are NaN
            p[:, 2] = np.where(keep, rs.choice(np.array([0.0, 0.7, 1.5], np.float32), n), rs.choice(np.array([-0.5, 1.6, np.nan], np.float32), n))
            clouds.append(dict(instance=r, stamp_ns=5 * S, points=p, transform=tf, origin=(1.1, -0.4, 0.25)))
            keeps.append(keep)
        fl.obs_buffer(clouds, 5 * S)
        ref.buffer(clouds, 5 * S)
        for r, n in enumerate(sizes):
            got, want = read_obs(fl, N, r), ref.observations(r)
            assert_same_obs(got, want, (pattern, n))
            assert len(got) == 1 and len(got[0]["points"]) == int(keeps[r].sum()), (pattern, n)  # the pattern is what was exercised


# ---------------------------------------------------------------------------------------------- 2. several clouds in one call
def _rand_cloud(rs, n):
    p = rs.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    p[:, 2] = rs.uniform(-0.6, 2.3, n).astype(np.float32)
    return p


def _scan(rs, n=720, rmin=0.3, rmax=6.0):
    r = rs.uniform(0.2, 2.0, n).astype(np.float32)
    return dict(ranges=r, angle_min=-math.pi, angle_increment=2 * math.pi / n, range_min=rmin, range_max=rmax)


SRC2 = [dict(observation_keep_time_ns=10 * S, min_obstacle_height=0.0, max_obstacle_height=2.0, obstacle_range=2.0, raytrace_range=2.5, flags=3),
        dict(observation_keep_time_ns=10 * S, min_obstacle_height=0.1, max_obstacle_height=1.0, obstacle_range=1.5, raytrace_range=3.0, flags=2)]


def test_several_clouds_in_one_call_and_sub_range(nav, N, dev_trig):
    A, B = make_fleet(nav, N, 3), make_fleet(nav, N, 3)
    try:
        A.obs_configure(SRC2, slots=2, max_cloud_points=300)
        ref = R.RefObsBuf(3, SRC2, 2, dev_trig)
        rs = np.random.RandomState(2)
        poses = [[1.6, 1.6, 0.2], [1.2, 1.9, -1.0], [2.0, 1.1, 2.5]]
        tf = [yaw_tf(p[2], p[0], p[1], 0.3) for p in poses]
        org = [(p[0], p[1], 0.3) for p in poses]
        clouds = [dict(instance=2, source=1, stamp_ns=1 * S, points=_rand_cloud(rs, 70), transform=tf[2], origin=org[2]),
                  dict(instance=0, source=0, stamp_ns=1 * S, points=_rand_cloud(rs, 257), transform=tf[0], origin=org[0]),
                  dict(instance=1, source=0, stamp_ns=2 * S, transform=tf[1], origin=org[1], **_scan(rs, 300)),
                  dict(instance=2, source=1, stamp_ns=2 * S, points=_rand_cloud(rs, 130), transform=tf[2], origin=org[2]),  # same (robot, source): the front
                  dict(instance=1, source=1, stamp_ns=2 * S, points=_rand_cloud(rs, 64), transform=tf[1], origin=org[1]),
                  dict(instance=0, source=1, stamp_ns=2 * S, points=np.zeros((0, 3), np.float32), transform=tf[0], origin=org[0])]
        A.obs_buffer(clouds, 2 * S)
        ref.buffer(clouds, 2 * S)
        for r in range(3):
            assert_same_obs(read_obs(A, N, r), ref.observations(r), r)
        o2 = ref.observations(2)
        assert [o["n_unfiltered"] for o in o2] == [130, 70]  # the later cloud of the call is the list's front
        assert [o["n_unfiltered"] for o in ref.observations(0)] == [257, 0]
        st = A.obs_status()
        assert [s.kept for s in st] == [2, 2, 2] and [s.evicted for s in st] == [0, 0, 0]
        assert [s.points for s in st] == [sum(len(o["points"]) for o in ref.observations(r)) for r in range(3)]
        # a sub-range with first > 0: robots 1 and 2 alone are staged and updated
        cur = A.obs_stage(poses[1:], 2 * S, first=1)
        assert cur.tolist() == [True, True]
        A.update_map(1, 2)
        B.stage_observations(poses[1:], ref.observations(1) + ref.observations(2), first=1)
        B.update_map(1, 2)
        for g in (N.GRID_MASTER, N.GRID_OBSTACLE):
            a, b = A.download(g), B.download(g)
            assert a.tobytes() == b.tobytes()
        assert (A.download(N.GRID_OBSTACLE)[1:] != 255).any() and (A.download(N.GRID_OBSTACLE)[0] == 255).all()
        assert A.bounds().tobytes() == B.bounds().tobytes()
    finally:
        A.close()
        B.close()


# ---------------------------------------------------------------------------------------------- 3. scans
def test_scans_bit_equal_with_device_trig_and_ulp_bound_with_host_trig(nav, N, dev_trig):
    fl = make_fleet(nav, N, 2)
    try:
        src = [dict(inf_is_valid=0, max_obstacle_height=2.0), dict(inf_is_valid=1, max_obstacle_height=2.0)]
        fl.obs_configure(src, slots=1, max_cloud_points=720)
        rs = np.random.RandomState(3)
        rmin, rmax = F32(0.45), F32(5.5)
        r = rs.uniform(0.5, 5.0, 720).astype(np.float32)
        r[5::37] = np.nan
        r[7::41] = np.inf
        r[11::43] = -np.inf
        r[13::47] = F32(0.44)                      # below range_min
        r[17::53] = rmin                           # at range_min: kept
        r[19::59] = rmax                           # at range_max: dropped
        r[23::61] = np.nextafter(rmax, F32(0))     # just under it: kept
        scan = dict(ranges=r, angle_min=-2.3561945, angle_increment=0.0065540750511, range_min=rmin, range_max=rmax)
        tf = yaw_tf(0.7, 1.5, 1.4, 0.4)
        clouds = [dict(instance=i, source=s, stamp_ns=S, transform=tf, origin=(1.5, 1.4, 0.4), **scan) for i in range(2) for s in range(2)]
        fl.obs_buffer(clouds, S)
        dev, host = R.RefObsBuf(2, src, 1, dev_trig), R.RefObsBuf(2, src, 1, R.host_trig)
        dev.buffer(clouds, S)
        host.buffer(clouds, S)
        got = [read_obs(fl, N, i) for i in range(2)]
        for i in range(2):
            assert_same_obs(got[i], dev.observations(i), i)  # bit-equal with the device's own trig
        n0, n1 = len(got[0][0]["points"]), len(got[0][1]["points"])
        assert n1 == n0 + int(np.isposinf(r).sum()) > n0 > 0 and n1 < 720  # exactly the +inf beams come back with the flag
        # against the host's libm: beams whose device sin and cos equal the host's bit for bit give bit-equal points, the others at
        # most one float ulp per coordinate.  The differing set is whatever navgpu_device_sincos shows in this run.
        for s in range(2):
            _, idx = R.project_scan(r, scan["angle_min"], scan["angle_increment"], rmin, rmax, s, R.host_trig)
            a = np.float64(F32(scan["angle_min"])) + idx.astype(np.float64) * np.float64(F32(scan["angle_increment"]))
            (dsn, dcs), (hsn, hcs) = dev_trig(a), R.host_trig(a)
            same = (dsn.view(np.uint64) == hsn.view(np.uint64)) & (dcs.view(np.uint64) == hcs.view(np.uint64))
            g, h = got[0][s]["points"], host.observations(0)[s]["points"]
            assert g.shape == h.shape == (len(idx), 3)  # z' does not depend on the trig: the same beams pass the height filter
            print(f"inf_is_valid={s}: {len(idx)} beams kept, {int((~same).sum())} with device trig != host trig, "
                  f"{int((g.view(np.uint32) != h.view(np.uint32)).any(axis=1).sum())} points differ")
            assert (g[same].view(np.uint32) == h[same].view(np.uint32)).all()
            ulp = np.spacing(np.maximum(np.abs(g), np.abs(h)).astype(np.float32))
            assert (np.abs(g.astype(np.float64) - h.astype(np.float64)) <= ulp.astype(np.float64)).all()
    finally:
        fl.close()


# ---------------------------------------------------------------------------------------------- 4. list behaviour
def test_list_behaviour_keep_time_eviction_and_is_current(nav, N, dev_trig):
    src = [dict(observation_keep_time_ns=2 * S, expected_update_rate_ns=S // 2), dict(observation_keep_time_ns=0)]
    fl = make_fleet(nav, N, 2)
    try:
        fl.obs_configure(src, slots=2, max_cloud_points=16)
        ref = R.RefObsBuf(2, src, 2, dev_trig)
        poses = [[1.6, 1.6, 0.0], [1.5, 1.7, 0.5]]

        def cloud(inst, source, stamp, tag):
            return dict(instance=inst, source=source, stamp_ns=stamp, points=np.array([[tag, 0.1, 0.5], [tag, 0.2, 0.6], [tag, 0.3, 9.0]], np.float32),
                        transform=yaw_tf(0.0, 1.0, 1.0, 0.0), origin=(1.0, 1.0, 0.0))

        def step(clouds, now, tags, current, evicted):
            if clouds:
                fl.obs_buffer(clouds, now)
                ref.buffer(clouds, now)
            cur = fl.obs_stage(poses, now)
            fl.update_map()  # (consumes the stage)
            for r in range(2):
                want = ref.observations(r)
                assert_same_obs(read_obs(fl, N, r), want, (now, r))
                assert [float(o["points"][0, 0]) - 1.0 for o in want] == tags[r], (now, r)  # the hand-worked expectation (x' = tag + 1)
            assert cur.tolist() == [ref.current(r, now) for r in range(2)] == current, now
            st = fl.obs_status()
            assert [s.evicted for s in st] == ref.evicted == evicted and [s.current for s in st] == [int(c) for c in current]

        # 1: first clouds everywhere
        step([cloud(0, 0, 10 * S, 1.0), cloud(0, 1, 10 * S, 2.0), cloud(1, 0, 10 * S, 3.0)], 10 * S, [[1.0, 2.0], [3.0]], [True, True], [0, 0])
        # 2: a second entry in the kept source; the keep-time-0 source holds its newest only
        step([cloud(0, 0, 11 * S, 4.0), cloud(0, 1, 11 * S, 5.0)], 11 * S, [[4.0, 1.0, 5.0], [3.0]], [True, False], [0, 0])
        # 3: robot 0's third live cloud in a ring of two slots - the oldest (exactly keep_time old, so not purged) is evicted;
        #    robot 1's first entry is exactly keep_time old: it stays behind the new one
        step([cloud(0, 0, 12 * S, 6.0), cloud(1, 0, 11 * S + S // 2, 7.0)], 12 * S, [[6.0, 4.0, 5.0], [7.0, 3.0]], [True, True], [1, 0])
        # 4: one ns later robot 1's old entry is past the keep time (the purge compares with last_updated: resetLastUpdated moves it)
        fl.obs_reset_last_updated(12 * S + 1, first=1, count=1)
        ref.reset_last_updated(12 * S + 1, [1])
        step([], 12 * S + 1, [[6.0, 4.0, 5.0], [7.0]], [True, True], [1, 0])
        # 5: isCurrent is <=: robot 0 was updated at 12 s, robot 1 at 12 s + 1 ns, the rate is 0.5 s
        step([], 12 * S + S // 2, [[6.0, 4.0, 5.0], [7.0]], [True, True], [1, 0])
        step([], 12 * S + S // 2 + 1, [[6.0, 4.0, 5.0], [7.0]], [False, True], [1, 0])
        # 6: ... and after resetLastUpdated both are current again (nothing is purged: 13 s - 11 s = the keep time)
        fl.obs_reset_last_updated(13 * S)
        ref.reset_last_updated(13 * S)
        step([], 13 * S, [[6.0, 4.0, 5.0], [7.0]], [True, True], [1, 0])
    finally:
        fl.close()


# ---------------------------------------------------------------------------------------------- 5. end-to-end equivalence
SRC_E2E = [dict(observation_keep_time_ns=S, min_obstacle_height=0.05, max_obstacle_height=1.9, obstacle_range=2.0, raytrace_range=2.5, flags=3),
           dict(observation_keep_time_ns=S, min_obstacle_height=0.0, max_obstacle_height=2.0, obstacle_range=1.8, raytrace_range=2.2, flags=3,
                inf_is_valid=1)]


def _assert_fleets_equal(A, B, N, voxel, what):
    for g in (N.GRID_MASTER, N.GRID_OBSTACLE) + ((N.GRID_VOXEL,) if voxel else ()):
        assert A.download(g).tobytes() == B.download(g).tobytes(), (what, g)
    assert A.bounds().tobytes() == B.bounds().tobytes(), what
    assert A.origins().tobytes() == B.origins().tobytes(), what
    if voxel:
        ea, eb = A.voxel_clearing_endpoints(), B.voxel_clearing_endpoints()
        for r in range(A.n):
            assert [len(x) for x in ea[r]] == [len(x) for x in eb[r]], (what, r)  # obs_counts
            for x, y in zip(ea[r], eb[r]):
                assert x.tobytes() == y.tobytes(), (what, r)
        return sum(len(x) for r in ea for x in r)
    return 0


def _cycle_clouds(rs, poses, stamp):
    clouds = []
    for i, p in enumerate(poses):
        tf, org = yaw_tf(p[2], p[0], p[1], 0.3), (p[0], p[1], 0.3)
        clouds.append(dict(instance=i, source=0, stamp_ns=stamp, points=_rand_cloud(rs, 150 + 57 * i), transform=tf, origin=org))
        sc = _scan(rs, 200, rmax=3.0)
        sc["ranges"][::17] = np.inf
        clouds.append(dict(instance=i, source=1, stamp_ns=stamp, transform=tf, origin=org, **sc))
    return clouds


@pytest.mark.parametrize("kind", ["obstacle", "rolling", "voxel"])
def test_end_to_end_equals_the_stage_path(nav, N, dev_trig, kind):
    layers = (N.LAYER_VOXEL if kind == "voxel" else N.LAYER_OBSTACLE) | N.LAYER_INFLATION
    kw = dict(layers=layers, max_points=1024, max_observations=4, rolling_window=(kind == "rolling"))
    A, B = make_fleet(nav, N, 2, **kw), make_fleet(nav, N, 2, **kw)
    try:
        if kind != "rolling":
            for f in (A, B):
                f.set_origin([[0.0, 0.0], [0.4, -0.2]])
        A.obs_configure(SRC_E2E, slots=2, max_cloud_points=256)
        ref = R.RefObsBuf(2, SRC_E2E, 2, dev_trig)
        rs = np.random.RandomState(5)
        ends = 0
        for cyc in range(4):
            now = (10 + cyc) * S // 2  # half a second apart with a keep time of 1 s: two entries per source from the second cycle on
            poses = [[1.6 + 0.11 * cyc, 1.5 + 0.07 * cyc, 0.3 * cyc], [1.9 - 0.09 * cyc, 1.3 + 0.05 * cyc, -0.4 * cyc]]
            clouds = _cycle_clouds(rs, poses, now)
            A.obs_buffer(clouds, now)
            ref.buffer(clouds, now)
            A.obs_stage(poses, now)
            want = ref.observations(0) + ref.observations(1)
            assert len(want) == (4 if cyc == 0 else 8)
            B.stage_observations(poses, want)
            A.update_map()
            B.update_map()
            ends += _assert_fleets_equal(A, B, N, kind == "voxel", (kind, cyc))
        obst = A.download(N.GRID_OBSTACLE)
        assert (obst == 254).any() and (obst == 0).any()  # something was marked and something cleared
        if kind == "voxel":
            assert ends > 0
        if kind == "rolling":
            assert (A.origins() != 0).any()
    finally:
        A.close()
        B.close()


# ---------------------------------------------------------------------------------------------- 6. set_global_frame
def test_set_global_frame(nav, N, dev_trig):
    A, B = make_fleet(nav, N, 2), make_fleet(nav, N, 2)
    try:
        A.obs_configure(SRC_E2E, slots=2, max_cloud_points=256)
        ref = R.RefObsBuf(2, SRC_E2E, 2, dev_trig)
        rs = np.random.RandomState(6)
        poses = [[1.3, 1.4, 0.2], [1.5, 1.2, -0.3]]
        for t in (10 * S, 10 * S + S // 2):
            clouds = _cycle_clouds(rs, poses, t)
            A.obs_buffer(clouds, t)
            ref.buffer(clouds, t)
        M = yaw_tf(0.4, 0.35, -0.15, 0.02)  # new_global <- global: a yaw and a translation
        A.obs_set_global_frame(M)
        ref.set_global_frame(M)
        for r in range(2):
            want = ref.observations(r)
            assert len(want) == 4
            assert_same_obs(read_obs(A, N, r), want, r)
        new_poses = [[1.6, 1.7, 0.6], [1.8, 1.4, 0.1]]
        A.obs_stage(new_poses, 10 * S + S // 2)
        B.stage_observations(new_poses, ref.observations(0) + ref.observations(1))
        A.update_map()
        B.update_map()
        _assert_fleets_equal(A, B, N, False, "after set_global_frame")
        # one robot only: the other's entries stay as they are
        before = snapshot(A, N)
        A.obs_set_global_frame(M, first=1, count=1)
        ref.set_global_frame(M, [1])
        after = snapshot(A, N)
        assert after[0] == before[0] and after[1] != before[1]
        assert_same_obs(read_obs(A, N, 1), ref.observations(1), "robot 1 alone")
    finally:
        A.close()
        B.close()


# ---------------------------------------------------------------------------------------------- 7. errors
def _raw_buffer(fl, N, clouds, now=0, **patch):
    arr, pts, rng = fl.pack_clouds(clouds)
    n_pts, n_rng = len(pts), len(rng)
    for k, v in patch.items():
        if k == "n_points":
            n_pts = v
        elif k == "n_ranges":
            n_rng = v
        else:
            setattr(arr[len(clouds) - 1], k, v)
    return fl.L.navgpu_obsbuf_buffer(fl.h, C.cast(arr, C.c_void_p), len(clouds), vp(pts) if len(pts) else None, n_pts, vp(rng) if len(rng) else None,
                                     n_rng, now)


def test_every_call_before_configure_is_a_state_error(nav, N):
    fl = make_fleet(nav, N, 2)
    try:
        L, h = fl.L, fl.h
        arr, pts, rng = fl.pack_clouds([dict(instance=0, stamp_ns=0, points=np.zeros((2, 3), np.float32))])
        poses = np.zeros((2, 3))
        obs, st, n = (N.Observation * 4)(), (N.ObsBufRobotStatus * 2)(), C.c_uint32()
        M = np.array(yaw_tf(0, 0, 0, 0) * 2, np.float64)
        assert L.navgpu_obsbuf_buffer(h, C.cast(arr, C.c_void_p), 1, vp(pts), 2, None, 0, 0) == STATE
        assert L.navgpu_obsbuf_stage(h, 0, 2, vp(poses), 0, None) == STATE
        assert L.navgpu_obsbuf_observations(h, 0, 0, C.cast(obs, C.c_void_p), 4, vp(pts), 2, C.byref(n)) == STATE
        assert L.navgpu_obsbuf_set_global_frame(h, 0, 2, vp(M)) == STATE
        assert L.navgpu_obsbuf_reset_last_updated(h, 0, 2, 0) == STATE
        assert L.navgpu_obsbuf_status(h, 0, 2, C.cast(st, C.c_void_p)) == STATE
    finally:
        fl.close()


def test_errors_leave_lists_and_staged_cycle_as_they_were(nav, N, dev_trig):
    src = [dict(observation_keep_time_ns=10 * S, min_obstacle_height=0.0, max_obstacle_height=1.0)]
    A, B = make_fleet(nav, N, 2, max_points=300, max_observations=2), make_fleet(nav, N, 2, max_points=300, max_observations=2)
    try:
        L = A.L
        sp = (N.ObsSourceParams * 9)(*[N.ObsSourceParams(**src[0]) for _ in range(9)])
        # configure: the limits
        assert L.navgpu_obsbuf_configure(A.h, C.cast(sp, C.c_void_p), 9, 1, 16) == INVALID      # n_sources > 8
        assert L.navgpu_obsbuf_configure(A.h, C.cast(sp, C.c_void_p), 0, 1, 16) == INVALID
        assert L.navgpu_obsbuf_configure(A.h, C.cast(sp, C.c_void_p), 1, 1, 65537) == INVALID   # max_cloud_points > 65536
        assert L.navgpu_obsbuf_configure(A.h, C.cast(sp, C.c_void_p), 1, 3, 16) == INVALID      # slots * n_sources > max_observations
        assert L.navgpu_obsbuf_configure(A.h, C.cast(sp, C.c_void_p), 2, 2, 16) == INVALID
        assert L.navgpu_obsbuf_status(A.h, 0, 1, C.cast((N.ObsBufRobotStatus * 1)(), C.c_void_p)) == STATE  # none of them configured anything
        A.obs_configure(src, slots=2, max_cloud_points=256)
        ref = R.RefObsBuf(2, src, 2, dev_trig)
        rs = np.random.RandomState(7)
        poses = [[1.6, 1.6, 0.0], [1.4, 1.8, 0.3]]
        tf = [yaw_tf(p[2], p[0], p[1], 0.2) for p in poses]
        good = [dict(instance=i, stamp_ns=S, points=_rand_cloud(rs, 120), transform=tf[i], origin=(poses[i][0], poses[i][1], 0.2)) for i in range(2)]
        A.obs_buffer(good, S)
        ref.buffer(good, S)
        A.obs_stage(poses, S)
        B.stage_observations(poses, ref.observations(0) + ref.observations(1))
        snap = snapshot(A, N)
        assert all(len(s) == 1 for s in snap)
        # a failed reconfigure under an allocation limit leaves the configuration, and its lists, in force
        A.set_alloc_limit(1024)
        assert L.navgpu_obsbuf_configure(A.h, C.cast(sp, C.c_void_p), 1, 1, 4096) == HIP
        A.set_alloc_limit(0)
        assert snapshot(A, N) == snap
        # buffer: each failing call buffers nothing - not even the good cloud in front of the bad one
        c = dict(instance=1, stamp_ns=2 * S, points=_rand_cloud(rs, 50), transform=tf[1], origin=(1.0, 1.0, 0.2))
        nan_tf, inf_org = list(tf[1]), (1.0, float("inf"), 0.2)
        nan_tf[4] = float("nan")
        big = dict(c, points=_rand_cloud(rs, 257))
        scan = dict(instance=1, stamp_ns=2 * S, transform=tf[1], **_scan(rs, 100))
        cases = [(_raw_buffer(A, N, [good[0], c], 2 * S, instance=2), INVALID), (_raw_buffer(A, N, [good[0], c], 2 * S, source=1), INVALID),
                 (_raw_buffer(A, N, [good[0], c], 2 * S, kind=2), INVALID), (_raw_buffer(A, N, [good[0], dict(c, transform=nan_tf)], 2 * S), INVALID),
                 (_raw_buffer(A, N, [good[0], dict(c, origin=inf_org)], 2 * S), INVALID), (_raw_buffer(A, N, [good[0], c], 2 * S, n_points=169), INVALID),
                 (_raw_buffer(A, N, [good[0], scan], 2 * S, n_ranges=99), INVALID), (_raw_buffer(A, N, [good[0], big], 2 * S), CAPACITY)]
        assert [rc for rc, _ in cases] == [w for _, w in cases]
        assert snapshot(A, N) == snap
        # stage: bad ranges, and the upper-bound capacity check - 2 x 200 unfiltered points against max_points = 300, although the
        # height filter leaves 40
        p = np.array(poses, np.float64)
        assert L.navgpu_obsbuf_stage(A.h, 1, 2, vp(p), S, None) == INVALID
        assert L.navgpu_obsbuf_stage(A.h, 0, 0, vp(p), S, None) == INVALID
        assert L.navgpu_obsbuf_stage(A.h, 0, 2, None, S, None) == INVALID
        tall = _rand_cloud(rs, 200)
        tall[:, 2] = 5.0
        tall[:20, 2] = 0.5
        two = [dict(instance=0, stamp_ns=3 * S, points=tall, transform=tf[0], origin=(1.6, 1.6, 0.2)),
               dict(instance=0, stamp_ns=3 * S + 1, points=tall, transform=tf[0], origin=(1.6, 1.6, 0.2))]
        A.obs_buffer(two, 3 * S + 1)
        ref.buffer(two, 3 * S + 1)
        snap2 = snapshot(A, N)
        assert [len(o[4]) // 12 for o in snap2[0]] == [20, 20] and A.obs_status()[0].evicted == 1
        assert L.navgpu_obsbuf_stage(A.h, 0, 2, vp(p), 3 * S + 1, None) == CAPACITY
        assert snapshot(A, N) == snap2
        for bad in (A.L.navgpu_obsbuf_set_global_frame(A.h, 0, 3, vp(np.zeros(36))), A.L.navgpu_obsbuf_reset_last_updated(A.h, 2, 1, 0),
                    A.L.navgpu_obsbuf_set_global_frame(A.h, 0, 1, vp(np.full(12, np.nan)))):
            assert bad == INVALID
        assert snapshot(A, N) == snap2
        # the cycle staged before all those failures is still the staged one
        A.update_map()
        B.update_map()
        _assert_fleets_equal(A, B, N, False, "after failed calls")
        # read-back capacities
        obs, n = (N.Observation * 2)(), C.c_uint32()
        buf = np.zeros((64, 3), np.float32)
        assert L.navgpu_obsbuf_observations(A.h, 0, 0, C.cast(obs, C.c_void_p), 1, vp(buf), 64, C.byref(n)) == CAPACITY
        assert L.navgpu_obsbuf_observations(A.h, 0, 0, C.cast(obs, C.c_void_p), 2, vp(buf), 39, C.byref(n)) == CAPACITY
        assert L.navgpu_obsbuf_observations(A.h, 2, 0, C.cast(obs, C.c_void_p), 2, vp(buf), 64, C.byref(n)) == INVALID
        assert L.navgpu_obsbuf_observations(A.h, 0, 0, C.cast(obs, C.c_void_p), 2, vp(buf), 40, C.byref(n)) == 2 and n.value == 40
    finally:
        A.close()
        B.close()


def test_rolling_stage_twice_is_a_state_error(nav, N, dev_trig):
    src = [dict(observation_keep_time_ns=0)]
    A = make_fleet(nav, N, 2, rolling_window=True)
    try:
        A.obs_configure(src, slots=1, max_cloud_points=64)
        rs = np.random.RandomState(8)
        poses = np.array([[1.6, 1.6, 0.0], [2.4, 1.8, 0.3]])
        A.obs_buffer([dict(instance=i, stamp_ns=S, points=_rand_cloud(rs, 40), transform=yaw_tf(0, *poses[i][:2], 0.2)) for i in range(2)], S)
        A.obs_stage(poses, S)
        org, snap = A.origins().copy(), snapshot(A, N)
        assert A.L.navgpu_obsbuf_stage(A.h, 0, 2, vp(poses + 0.5), S, None) == STATE  # the staged shift is not consumed yet
        assert A.origins().tobytes() == org.tobytes() and snapshot(A, N) == snap
        A.update_map()
        A.obs_stage(poses + 0.5, S)  # consumed: the next stage is accepted
        A.update_map()
        assert (A.origins() != org).any()
    finally:
        A.close()


# ---------------------------------------------------------------------------------------------- 8. determinism
def _determinism_run(nav, N):
    fl = make_fleet(nav, N, 3)
    try:
        fl.obs_configure(SRC_E2E, slots=2, max_cloud_points=1024)
        rs = np.random.RandomState(9)
        poses = [[1.6, 1.6, 0.1], [1.2, 1.9, -1.0], [2.0, 1.1, 2.5]]
        for t in (10 * S, 10 * S + S // 3, 10 * S + 2 * S // 3):
            clouds = _cycle_clouds(rs, poses, t)
            clouds.append(dict(instance=1, source=0, stamp_ns=t, points=_rand_cloud(rs, 1000), transform=yaw_tf(0.2, 1.0, 1.0, 0.1)))
            fl.obs_buffer(clouds, t)
        fl.obs_set_global_frame(yaw_tf(0.1, 0.2, 0.3, 0.0), first=0, count=2)
        return snapshot(fl, N)
    finally:
        fl.close()


def test_two_fresh_fleets_hold_identical_ring_bytes(nav, N):
    a, b = _determinism_run(nav, N), _determinism_run(nav, N)
    assert a == b
    assert sum(len(o[4]) for r in a for o in r) > 0
