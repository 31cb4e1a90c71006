"""CPU-side checks for the voxel-layer debug outputs (navgpu_voxel_points, navgpu_voxel_clearing_endpoints): the restatements of
tests/voxel_export_ref.py - the yardstick of tests/test_gpu_voxel_export.py - are pinned against the reference's own
voxel_grid test expectation and against the CPU oracle's voxel layer, and the two entry points are declared, exported and
bound.  No GPU."""
import os
import re

import numpy as np
import pytest

import voxel_export_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mark(cols, x, y, z):  # VoxelGrid::markVoxel (voxel_grid.h:85-95)
    cols[y, x] |= np.uint32((1 << z << 16) | (1 << z))


def _clear(cols, x, y, z):  # VoxelGrid::clearVoxel (:131-140)
    cols[y, x] &= np.uint32(~((1 << z << 16) | (1 << z)) & 0xFFFFFFFF)


def test_get_voxel_matches_the_reference_tabletop_test():
    """voxel_grid/test/voxel_grid_tests.cpp, basicMarkingAndClearing: a 50 x 10 x 16 grid, an 11 x 4 table at z = 12"""
    sx, sy, sz, table_z = 50, 10, 16, 12
    cols = np.full((sy, sx), 0x0000FFFF, np.uint32)  # VoxelGrid::reset (voxel_grid.cpp:54): everything unknown
    for x in range(5, 16):
        for y in range(0, 4):
            _mark(cols, x, y, table_z)
    st = R.get_voxel(cols, sz)
    assert (st[0:4, 5:16, table_z] == R.MARKED).all()
    assert (st == R.MARKED).sum() == 44 and (st == R.UNKNOWN).sum() == sx * sy * sz - 44 and (st == R.FREE).sum() == 0
    for x in range(5, 16):  # clearVoxelLine along the row y = 0
        _clear(cols, x, 0, table_z)
    st = R.get_voxel(cols, sz)
    assert (st == R.MARKED).sum() == 33 and (st == R.FREE).sum() == 11 and (st == R.UNKNOWN).sum() == sx * sy * sz - 44
    assert (st[0, 5:16, table_z] == R.FREE).all()
    # the clouds: as many points as voxels, y outer / x / z inner, cell centres
    pts = R.voxel_points(cols, R.MARKED, sz, -1.0, 2.0, 0.05, 0.1, 0.2, True)
    assert pts.shape == (33, 3)
    assert tuple(pts[0]) == (-1.0 + 5.5 * 0.05, 2.0 + 1.5 * 0.05, 0.1 + 12.5 * 0.2)
    assert tuple(pts[11]) == (-1.0 + 5.5 * 0.05, 2.0 + 2.5 * 0.05, 0.1 + 12.5 * 0.2)
    unk = R.voxel_points(cols, R.UNKNOWN, sz, 0.0, 0.0, 1.0, 0.0, 1.0, False)
    assert unk.dtype == np.float32 and tuple(unk[0]) == (0.5, 0.5, 0.5) and tuple(unk[1]) == (0.5, 0.5, 1.5) and tuple(unk[16]) == (1.5, 0.5, 0.5)
    assert len(R.voxel_points(cols, R.UNKNOWN, 10, 0.0, 0.0, 1.0, 0.0, 1.0, False)) == sx * sy * 10  # z < z_voxels only


def test_zmask_edges():
    cols = np.array([[0xFFFFFFFF, 0x80008000, 0x00018001]], np.uint32)
    assert (R.get_voxel(cols, 16)[0, 0] == R.MARKED).all()
    assert R.get_voxel(cols, 16)[0, 1].tolist() == [0] * 15 + [R.MARKED]
    assert R.get_voxel(cols, 1)[0].ravel().tolist() == [R.MARKED, R.FREE, R.MARKED]
    assert R.get_voxel(cols, 16)[0, 2].tolist() == [R.MARKED] + [0] * 14 + [R.UNKNOWN]


def _oracle(orc, robot, **vox):
    o = orc.LayeredCostmap(False)
    ox, oy = R.END_ORIGINS[robot]
    o.resize(R.END_NX, R.END_NY, R.END_RES, ox, oy)
    o.add_voxel(footprint_clearing=False, max_obstacle_height=R.END_MAX_H, z_voxels=R.END_Z_VOXELS, origin_z=R.END_ORIGIN_Z,
                z_resolution=R.END_Z_RES, **vox)
    return o


@pytest.mark.parametrize("robot", [0, 1])
def test_marked_set_projects_onto_the_oracles_lethal_cells(orc, robot):
    """mark_threshold 0: a column with any MARKED voxel is LETHAL in the layer's 2-D grid, and no other cell is"""
    o = _oracle(orc, robot, unknown_threshold=15, mark_threshold=0)
    for ob in R.end_observations(robot)[:2]:
        o.add_observation(ob["points"], origin=ob["origin"], obstacle_range=ob["obstacle_range"], raytrace_range=ob["raytrace_range"],
                          marking=ob["marking"], clearing=ob["clearing"])
    o.update_map(*R.END_ORIGINS[robot], 0.0)
    st = R.get_voxel(o.voxels(), R.END_Z_VOXELS)
    lethal = o.layer(2) == 254
    assert lethal.sum() > 20
    assert np.array_equal((st == R.MARKED).any(axis=2), lethal)
    g = R.end_geometry(robot)
    pts = R.voxel_points(o.voxels(), R.MARKED, R.END_Z_VOXELS, g.ox, g.oy, g.res, g.origin_z, g.z_res, True)
    cells = {(int((x - g.ox) / g.res), int((y - g.oy) / g.res)) for x, y, _ in pts}
    assert cells == {(int(x), int(y)) for y, x in zip(*np.nonzero(lethal))}


@pytest.mark.parametrize("robot", [0, 1])
def test_clip_restatement_reproduces_the_oracles_cleared_voxels(orc, robot):
    """The restated clip against the oracle's grid: a fresh voxel layer (every voxel UNKNOWN) after ONE clearing observation
    holds exactly the voxels that ClearVoxel walks from the sensor to the restated endpoints clear.  A wrong or missing
    endpoint clears other voxels."""
    g = R.end_geometry(robot)
    pts, sensor = R.end_cloud(robot)
    o = _oracle(orc, robot, unknown_threshold=15, mark_threshold=0)
    o.add_observation(pts, origin=sensor, obstacle_range=2.5, raytrace_range=100.0, marking=False, clearing=True)
    o.update_map(*R.END_ORIGINS[robot], 0.0)
    r = R.clearing_endpoints(g, pts, sensor)
    assert r["sensor"] is not None
    cols = np.full(g.nx * g.ny, 0x0000FFFF, np.uint32)
    for px, py, pz in r["cells"]:
        R.clear_voxel_line(cols, g.nx, *r["sensor"], px, py, pz, max_length=int(100.0 / g.res))
    assert np.array_equal(cols.reshape(g.ny, g.nx), o.voxels())
    # the inputs hold what they are meant to hold, and their decisions have the margin the GPU comparison needs
    on_threshold = R.assert_decisions_have_margin(r)
    assert 0 < len(r["kept"]) <= len(pts) and on_threshold >= 6  # (rays cut at x = origin_x, y = origin_y and the floor)
    kept = set(r["kept"])
    assert {12, 13, 14, 15} <= kept  # nearer than 2 * res: scaling_fact 0, the endpoint is the sensor itself
    for i in (12, 13, 14, 15):
        assert r["ends"][r["kept"].index(i)] == tuple(np.float64(v) for v in sensor)
    ends = dict(zip(r["kept"], r["ends"]))
    for i in (0, 1):  # above max_obstacle_height: cut at max_obstacle_height - 0.01
        assert abs(ends[i][2] - (R.END_MAX_H - 0.01)) < 1e-12
    for i in (6, 7):  # beyond map_end_x = origin + (size - 0.5) * res
        assert abs(ends[i][0] - (g.ox + (g.nx - 0.5) * g.res)) < 1e-12
    for i in (10, 11):
        assert abs(ends[i][1] - (g.oy + (g.ny - 0.5) * g.res)) < 1e-12


def test_larger_clouds_of_the_gpu_test_keep_the_margin():
    g = R.end_geometry(0)
    for n, seed in ((600, 1), (300, 2)):
        pts, sensor = R.end_cloud(0, n=n, seed=seed)
        r = R.clearing_endpoints(g, pts, sensor)
        R.assert_decisions_have_margin(r)
        assert len(r["kept"]) > (512 if n == 600 else 256)
    pts, sensor = R.end_cloud(0, n=300, seed=2)
    r = R.clearing_endpoints(g, pts, (sensor[0] - 0.4, sensor[1] + 0.3, 0.35))  # the second sensor of that test
    R.assert_decisions_have_margin(r)
    assert len(r["kept"]) > 256


def test_observation_without_endpoints():
    g = R.end_geometry(0)
    obs = R.end_observations(0)
    assert R.clearing_endpoints(g, obs[2]["points"], obs[2]["origin"])["kept"] == []       # sensor origin off the map
    assert R.clearing_endpoints(g, np.zeros((0, 3), np.float32), obs[0]["origin"])["kept"] == []  # no points


def test_entry_points_are_declared_exported_and_bound():
    import navigation_amd as nav
    from navigation_amd import _lib
    if not os.path.exists(nav.lib_path()):
        nav.build()
    L = nav.lib()
    header = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert re.search(r"\bint navgpu_voxel_points\(navgpu_fleet\* \w+, uint32_t first, uint32_t count, int status, int as_double,\s*uint32_t capacity,"
                     r"\s*void\* xyz,\s*uint32_t\* counts\);", header)
    assert re.search(r"\bint navgpu_voxel_clearing_endpoints\(navgpu_fleet\* \w+, uint32_t first, uint32_t count, uint32_t capacity,\s*float\* xyz,"
                     r"\s*uint32_t\* obs_counts, uint32_t\* counts\);", header)
    assert len(bound["navgpu_voxel_points"]) == 8 and len(bound["navgpu_voxel_clearing_endpoints"]) == 7
    for name in ("navgpu_voxel_points", "navgpu_voxel_clearing_endpoints"):
        assert hasattr(L, name), name
    assert re.search(r"#define NAVGPU_VOXEL_UNKNOWN 1\b", header) and re.search(r"#define NAVGPU_VOXEL_MARKED 2\b", header)
    assert (_lib.VOXEL_UNKNOWN, _lib.VOXEL_MARKED) == (R.UNKNOWN, R.MARKED) == (1, 2)
    assert L.navgpu_kernel_name(_lib.K_VOXEL_EXPORT) == b"k_voxel_export"
    # argument checks come before anything touches a device
    assert L.navgpu_voxel_points(None, 0, 1, 2, 0, 0, None, None) == -1
    assert L.navgpu_voxel_clearing_endpoints(None, 0, 1, 0, None, None, None) == -1
