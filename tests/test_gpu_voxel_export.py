"""navgpu_voxel_points and navgpu_voxel_clearing_endpoints through the C-ABI, compared with == against the restatements of
tests/voxel_export_ref.py (pinned on the CPU by tests/test_voxel_export_host.py) applied to navgpu_grid_download(
NAVGPU_GRID_VOXEL) and navgpu_fleet_get_origin of the same fleet: counts, element-for-element order, and the float / double
bits of every coordinate.  Voxel centres are exact; the clipped ray ends are the same unfused fp64 sequence on both sides,
so they are asserted bit-equal after narrowing to float.  Need a real MI355X.

The count / emit launches take 1024 columns per chunk (256 lanes x 4 columns) and the scan 256 chunk totals per tile."""
import ctypes as C

import numpy as np
import pytest

import voxel_export_ref as R

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -5
RES = 0.05
FP = [[0.1, 0.1], [-0.1, 0.1], [-0.1, -0.1], [0.1, -0.1]]
GUARD = 12345.0


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


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw_points(fl, status, as_double, first, count, capacity):
    """one navgpu_voxel_points call into a buffer preset to GUARD, with one guard element behind it -> (rc, counts, buffer)"""
    dt = np.float64 if as_double else np.float32
    flat = np.full(count * capacity * 3 + 1, GUARD, dt)
    counts = np.full(count, 0xDEAD, np.uint32)
    rc = fl.L.navgpu_voxel_points(fl.h, first, count, status, int(as_double), capacity, vp(flat) if capacity else None, vp(counts))
    return rc, counts, flat


def _expected_points(fl, N, status, as_double, z_voxels, origin_z=0.0, z_res=0.2, first=0, count=None):
    vox = fl.download(N.GRID_VOXEL)
    org = fl.origins()
    count = fl.n - first if count is None else count
    return [R.voxel_points(vox[i], status, z_voxels, org[i, 0], org[i, 1], fl.res, origin_z, z_res, as_double) for i in range(first, first + count)]


def _check_points(fl, N, status, as_double, z_voxels, first=0, count=None, **geo):
    want = _expected_points(fl, N, status, as_double, z_voxels, first=first, count=count, **geo)
    got = fl.voxel_points(status, as_double=as_double, first=first, count=count)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), ("robot", k)
    return want


def _cloud(rs, nx, ny, n, ox=0.0, oy=0.0):
    return np.stack([rs.uniform(ox + 0.05, ox + nx * RES - 0.05, n), rs.uniform(oy + 0.05, oy + ny * RES - 0.05, n), rs.uniform(0.05, 1.95, n)],
                    axis=1).astype(np.float32)


def _voxel_fleet(nav, N, n, nx, ny, z_voxels=10, origin_z=0.0, z_res=0.2, max_points=512, max_observations=2, **kw):
    fl = nav.Fleet(n, nx, ny, RES, layers=N.LAYER_VOXEL, track_unknown=True, max_points=max_points, max_observations=max_observations, **kw)
    fl.configure_obstacle(z_voxels=z_voxels, origin_z=origin_z, z_resolution=z_res, max_obstacle_height=2.0)
    fl.set_footprint(FP)
    return fl


def _update(fl, clouds, poses=None):
    """one update with one marking + clearing cloud per robot, the sensor in the middle of the map at 1.1 m"""
    org = fl.origins()
    poses = [[org[i, 0] + fl.nx * RES / 2, org[i, 1] + fl.ny * RES / 2, 0.0] for i in range(fl.n)] if poses is None else poses
    obs = [dict(instance=i, points=c, origin=(poses[i][0] + 0.013, poses[i][1] - 0.021, 1.1), obstacle_range=50.0, raytrace_range=50.0)
           for i, c in enumerate(clouds)]
    fl.stage_observations(poses, obs)
    fl.update_map()


# ---------------------------------------------------------------------------------------------- voxel points
@pytest.fixture(scope="module")
def small(nav, N):
    """37 x 29 cells = 1073 columns: two chunks, the second of 49 columns; a row of 37 straddles lanes, waves and the chunk"""
    fl = _voxel_fleet(nav, N, 3, 37, 29, origin_z=0.1, z_res=0.19)
    fl.set_origin([[-1.0, 0.5], [0.3, -2.2], [10.05, 7.0]])
    rs = np.random.RandomState(1)
    _update(fl, [_cloud(rs, 37, 29, n, *o) for n, o in zip((40, 170, 400), fl.origins())])
    yield fl
    fl.close()


@pytest.mark.parametrize("as_double", [False, True])
@pytest.mark.parametrize("status", [R.UNKNOWN, R.MARKED])
def test_points_equal_restatement(small, N, status, as_double):
    want = _check_points(small, N, status, as_double, 10, origin_z=0.1, z_res=0.19)
    n = [len(w) for w in want]
    assert len(set(n)) == 3 and min(n) > 0, n  # the robots' counts differ
    if status == R.UNKNOWN:
        assert max(n) < 37 * 29 * 10  # something was cleared or marked


def test_points_of_a_sub_range(small, N):
    for status in (R.UNKNOWN, R.MARKED):
        _check_points(small, N, status, False, 10, first=1, count=2, origin_z=0.1, z_res=0.19)


def test_points_capacity_count_only_and_determinism(small, N):
    want = _expected_points(small, N, R.MARKED, True, 10, origin_z=0.1, z_res=0.19)
    n = np.array([len(w) for w in want], np.uint32)
    # counts only
    rc, counts, flat = _raw_points(small, R.MARKED, True, 0, 3, 0)
    assert rc == OK and np.array_equal(counts, n) and flat[0] == GUARD
    # a capacity below the smallest count: true counts, the head of the full answer, nothing behind a robot's block or the buffer
    cap = int(n.min()) - 3
    assert cap > 0
    rc, counts, flat = _raw_points(small, R.MARKED, True, 0, 3, cap)
    assert rc == OK and np.array_equal(counts, n)
    for k in range(3):
        assert flat[k * cap * 3:(k + 1) * cap * 3].tobytes() == want[k][:cap].tobytes(), k
    assert flat[-1] == GUARD
    # a capacity between the counts: the short robots' blocks keep the caller's bytes behind their last point
    cap = int(np.sort(n)[1])
    rc, counts, flat = _raw_points(small, R.MARKED, True, 0, 3, cap)
    assert rc == OK and np.array_equal(counts, n)
    for k in range(3):
        here = min(int(n[k]), cap)
        block = flat[k * cap * 3:(k + 1) * cap * 3]
        assert block[:here * 3].tobytes() == want[k][:here].tobytes(), k
        assert (block[here * 3:] == GUARD).all(), k
    assert flat[-1] == GUARD
    # two identical calls give identical bytes
    rc2, counts2, flat2 = _raw_points(small, R.MARKED, True, 0, 3, cap)
    assert rc2 == OK and counts2.tobytes() == counts.tobytes() and flat2.tobytes() == flat.tobytes()
    a = small.voxel_points(R.UNKNOWN)
    b = small.voxel_points(R.UNKNOWN)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("z_voxels", [1, 16])
def test_zmask_edges(nav, N, z_voxels):
    fl = _voxel_fleet(nav, N, 1, 20, 20, z_voxels=z_voxels, z_res=2.0 / z_voxels)
    rs = np.random.RandomState(z_voxels)
    _update(fl, [_cloud(rs, 20, 20, 60)])
    for status in (R.UNKNOWN, R.MARKED):
        for as_double in (False, True):
            want = _check_points(fl, N, status, as_double, z_voxels, z_res=2.0 / z_voxels)
            assert len(want[0]) > 0
    fl.close()


def test_fresh_fleet_is_all_unknown(nav, N):
    fl = _voxel_fleet(nav, N, 2, 37, 29)
    assert (fl.download(N.GRID_VOXEL) == 0x0000FFFF).all()
    rc, counts, _ = _raw_points(fl, R.UNKNOWN, False, 0, 2, 0)
    assert rc == OK and counts.tolist() == [37 * 29 * 10] * 2
    _check_points(fl, N, R.UNKNOWN, False, 10)
    rc, counts, flat = _raw_points(fl, R.MARKED, False, 0, 2, 5)
    assert rc == OK and counts.tolist() == [0, 0] and (flat == GUARD).all()  # nothing is written
    fl.close()


def test_scan_carries_across_tiles(nav, N):
    """300 x 260 = 78 000 columns = 77 chunks: more totals than one wave holds.  The scan's carry across its 256-total tiles
    needs more than 256 chunks, so a second map of 600 x 450 = 270 000 columns = 264 chunks follows (enlarged for that reason)."""
    for nx, ny, n_pts in ((300, 260, 300), (600, 450, 500)):
        assert (nx * ny + 1023) // 1024 > (64 if nx == 300 else 256)
        fl = _voxel_fleet(nav, N, 1, nx, ny)
        rs = np.random.RandomState(nx)
        _update(fl, [_cloud(rs, nx, ny, n_pts)])  # sparse marks
        want = _check_points(fl, N, R.MARKED, False, 10)
        assert 0 < len(want[0]) <= n_pts
        rows = ((want[0][:, 1].astype(np.float64)) / RES).astype(int)
        assert rows.min() < ny // 4 and rows.max() > 3 * ny // 4  # marks in the first and the last chunks
        _check_points(fl, N, R.UNKNOWN, True, 10)
        fl.close()


def test_rolling_window(nav, N):
    fl = _voxel_fleet(nav, N, 2, 37, 29, rolling_window=True)
    rs = np.random.RandomState(5)
    poses = [[0.9, 0.7, 0.0], [1.0, 0.8, 0.0]]
    _update(fl, [_cloud(rs, 37, 29, 80), _cloud(rs, 37, 29, 90)], poses=poses)
    org0 = fl.origins().copy()
    before = _check_points(fl, N, R.MARKED, True, 10)
    # the window moves: between the stage and the update the grids lag the origins
    poses2 = [[poses[0][0] + 0.33, poses[0][1] - 0.17, 0.0], [poses[1][0] - 0.26, poses[1][1] + 0.41, 0.0]]
    fl.stage_observations(poses2, [])
    counts = np.zeros(2, np.uint32)
    assert fl.L.navgpu_voxel_points(fl.h, 0, 2, R.MARKED, 0, 0, None, vp(counts)) == STATE
    per_obs = np.zeros((2, 2), np.uint32)
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 0, 2, 0, None, vp(per_obs), vp(counts)) == STATE
    fl.update_map()
    org1 = fl.origins()
    assert (org1 != org0).all()
    after = _check_points(fl, N, R.MARKED, True, 10)  # == the restatement with the shifted origin
    for k in range(2):  # the marks that stayed inside the window kept their world coordinates
        a = {tuple(np.round(p, 6)) for p in after[k]}
        assert len(a) > 0 and a <= {tuple(np.round(p, 6)) for p in before[k]}
    fl.close()


def test_points_argument_errors(nav, N, small):
    counts = np.zeros(4, np.uint32)
    buf = np.zeros(64 * 3 * 4, np.float64)
    L, h = small.L, small.h
    assert L.navgpu_voxel_points(h, 0, 3, 0, 0, 0, None, vp(counts)) == INVALID   # FREE is never returned
    assert L.navgpu_voxel_points(h, 0, 3, 3, 0, 0, None, vp(counts)) == INVALID
    assert L.navgpu_voxel_points(h, 0, 4, R.MARKED, 0, 0, None, vp(counts)) == INVALID  # range outside the fleet
    assert L.navgpu_voxel_points(h, 3, 1, R.MARKED, 0, 0, None, vp(counts)) == INVALID
    assert L.navgpu_voxel_points(h, 0, 0, R.MARKED, 0, 0, None, vp(counts)) == INVALID
    assert L.navgpu_voxel_points(h, 0, 3, R.MARKED, 0, 4, None, vp(counts)) == INVALID  # a capacity without a buffer
    assert L.navgpu_voxel_points(h, 0, 3, R.MARKED, 0, 0, None, None) == INVALID
    per_obs = np.zeros((4, 2), np.uint32)
    assert L.navgpu_voxel_clearing_endpoints(h, 0, 4, 0, None, vp(per_obs), vp(counts)) == INVALID
    assert L.navgpu_voxel_clearing_endpoints(h, 0, 3, 0, None, None, vp(counts)) == INVALID
    fl = nav.Fleet(2, 20, 20, RES, layers=N.LAYER_OBSTACLE)  # no voxel layer
    assert fl.L.navgpu_voxel_points(fl.h, 0, 2, R.MARKED, 0, 64, vp(buf), vp(counts)) == INVALID
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 0, 2, 0, None, vp(per_obs), vp(counts)) == INVALID
    fl.close()


# ---------------------------------------------------------------------------------------------- clearing endpoints
def _end_fleet(nav, N, n=2, max_points=256, max_observations=4):
    fl = nav.Fleet(n, R.END_NX, R.END_NY, R.END_RES, layers=N.LAYER_VOXEL, track_unknown=True, max_points=max_points,
                   max_observations=max_observations)
    fl.configure_obstacle(z_voxels=R.END_Z_VOXELS, origin_z=R.END_ORIGIN_Z, z_resolution=R.END_Z_RES, max_obstacle_height=R.END_MAX_H)
    fl.set_footprint(FP)
    fl.set_origin(R.END_ORIGINS[:n])
    return fl


def _expected_endpoints(robot, observations):
    """per observation the float32 (k, 3) cloud of the restatement; asserts the margin of every decision first"""
    g = R.end_geometry(robot)
    out = []
    for ob in observations:
        if not ob.get("clearing", True):
            out.append(np.zeros((0, 3), np.float32))
            continue
        r = R.clearing_endpoints(g, ob["points"], ob["origin"])
        R.assert_decisions_have_margin(r)
        out.append(np.array(r["ends"], np.float64).reshape(-1, 3).astype(np.float32))  # Point32
    return out


def _compare_endpoints(got, want):
    """bit-equal first; the figures of a difference (largest ulp distance, share of points) are in the message"""
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    share = float((ulps.max(axis=1) > 0).mean()) if len(ulps) else 0.0
    print("clearing endpoints differ: max ulp", int(ulps.max()), "share of points", share)
    assert False, f"clearing endpoints are not bit-equal: max {int(ulps.max())} float ulp, {share:.4%} of {len(got)} points"


def test_clearing_endpoints_equal_restatement(nav, N):
    fl = _end_fleet(nav, N)
    obs = [R.end_observations(r) for r in range(2)]
    poses = [[o[0] + 1.5, o[1] + 1.5, 0.0] for o in R.END_ORIGINS]
    staged = [dict(ob, instance=r) for r in range(2) for ob in obs[r]]
    fl.stage_observations(poses, staged)
    counts = np.zeros(2, np.uint32)
    per_obs = np.zeros((2, 4), np.uint32)
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 0, 2, 0, None, vp(per_obs), vp(counts)) == STATE  # staged, not updated yet
    fl.update_map()
    assert np.allclose(fl.origins(), R.END_ORIGINS, rtol=0, atol=0)
    want = [_expected_endpoints(r, obs[r]) for r in range(2)]
    # counts only
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 0, 2, 0, None, vp(per_obs), vp(counts)) == OK
    assert per_obs.tolist() == [[len(w) for w in want[r]] + [0] for r in range(2)]
    assert counts.tolist() == [sum(len(w) for w in want[r]) for r in range(2)]
    assert per_obs[:, 0].min() > 100 and (per_obs[:, 1:] == 0).all()  # marking-only, sensor off the map, not staged
    got = fl.voxel_clearing_endpoints()
    for r in range(2):
        assert [len(c) for c in got[r]] == per_obs[r].tolist()
        _compare_endpoints(got[r][0], want[r][0])  # cloud order
    # capacity below the count, guard behind the buffer, a sub-range, two identical calls
    cap = 50
    flat = np.full(cap * 3 + 1, GUARD, np.float32)
    one = np.zeros(1, np.uint32)
    per1 = np.zeros((1, 4), np.uint32)
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 1, 1, cap, vp(flat), vp(per1), vp(one)) == OK
    assert one[0] == counts[1] and per1[0].tolist() == per_obs[1].tolist() and flat[-1] == GUARD
    assert flat[:-1].tobytes() == got[1][0][:cap].tobytes()
    again = fl.voxel_clearing_endpoints()
    assert all(a.tobytes() == b.tobytes() for r in range(2) for a, b in zip(again[r], got[r]))
    # the next stage invalidates them until its update
    fl.stage_observations(poses, [])
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 0, 2, 0, None, vp(per_obs), vp(counts)) == STATE
    fl.update_map()
    assert fl.L.navgpu_voxel_clearing_endpoints(fl.h, 0, 2, 0, None, vp(per_obs), vp(counts)) == OK and counts.tolist() == [0, 0]
    fl.close()


def test_clearing_endpoints_across_point_chunks_and_update_bounds(nav, N):
    """two clearing observations of 600 and 300 points (3 and 2 chunks of 256 points) for one robot, consumed by
    navgpu_obstacle_update_bounds instead of an update"""
    fl = _end_fleet(nav, N, n=1, max_points=1024, max_observations=2)
    pts_a, sensor = R.end_cloud(0, n=600, seed=1)
    pts_b, _ = R.end_cloud(0, n=300, seed=2)
    obs = [dict(points=pts_a, origin=sensor, marking=False, clearing=True), dict(points=pts_b, origin=(sensor[0] - 0.4, sensor[1] + 0.3, 0.35), clearing=True)]
    fl.stage_observations([[0.5, 2.0, 0.0]], [dict(ob, instance=0) for ob in obs])
    bounds = np.array([[1e30, 1e30, -1e30, -1e30]], np.float64)
    assert fl.L.navgpu_obstacle_update_bounds(fl.h, 0, 1, vp(bounds)) == OK
    want = _expected_endpoints(0, obs)
    got = fl.voxel_clearing_endpoints()
    assert [len(c) for c in got[0]] == [len(w) for w in want] and len(want[0]) > 512 and len(want[1]) > 256
    for g, w in zip(got[0], want):
        _compare_endpoints(g, w)
    fl.close()
