"""navgpu_costmap3d_* on the device against the numpy yardstick (tests/costmap3d_ref.py): the same cells, mesh and poses on both sides.

Verdicts (collides or not) must be equal, distances within 1e-9 m: the coordinates stay below 64 m, where a double's ulp is 1.4e-14,
so two evaluation orders of a few dozen operations differ by less than 1e-12; 1e-9 leaves three orders of margin.  The small maps
are 72 x 8 x 64 cells of 0.25 m at origins that are multiples of it - every coordinate is exact in binary, touching cases
included - so that x crosses a 64-column chunk of the walk and z uses bit 63."""
import os

import numpy as np
import pytest

import costmap3d_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "costmap3d")
TOL = 1e-9
RES = 0.25
ORIGIN = np.array([-2.0, 1.0, -0.5])
SX, SY, SZ = 72, 8, 64
CORNER_CELLS = [(0, 0, 0), (71, 7, 63), (0, 7, 63), (71, 0, 0), (35, 3, 31)]
MESHES = {"tetra": (ref.TETRA_VERTICES, ref.TETRA_TRIANGLES), "cube": (ref.CUBE_VERTICES, ref.CUBE_TRIANGLES)}


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def small_map(nav, n_instances=1, **kw):
    c = nav.Costmap3D(n_instances, SX, SY, SZ, RES, max_triangles=16, max_boxes=256, max_poses=256, **kw)
    for i in range(n_instances):
        c.set_origin(i, ORIGIN)
    return c


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    return list(a / np.linalg.norm(a) * np.sin(angle / 2)) + [np.cos(angle / 2)]


def pose_at(xyz, q=(0.0, 0.0, 0.0, 1.0)):
    return list(xyz) + list(q)


def expected(cells, origin, mesh, poses, mode, regions=None, scale=(0.0, 0.0, 0.0), limit=ref.DBL_MAX):
    centres = ref.cell_centres(cells, origin, RES) if len(cells) else np.zeros((0, 3))
    regions = [ref.ALL] * len(poses) if regions is None else regions
    return np.array([ref.query_pose(centres, RES, mesh[0], mesh[1], np.asarray(p, np.float64), mode=mode, region=int(r), scale=scale, limit=limit)
                     for p, r in zip(poses, regions)])


def assert_costs(got, want):
    assert np.array_equal(got < 0, want < 0), (got, want)
    free = want >= 0
    assert np.all(np.abs(got[free] - want[free]) <= TOL), (got, want)
    assert np.array_equal(got[~free], want[~free])


def poses_around(cell, origin=ORIGIN):
    """poses that put the mesh's corner at, near and away from a cell: touching faces, edges and vertices, overlapping, rotated"""
    lo = origin + np.asarray(cell) * RES
    out = []
    for d in ([0.0, 0.0, 0.0], [RES, 0.0, 0.0], [RES, RES, 0.0], [RES, RES, RES], [0.5, 0.0, 0.0], [0.75, 0.5, 0.0], [0.5, 0.75, 1.0],
              [-1.0, 0.0, 0.0], [-1.25, 0.0, 0.0], [-1.5, -1.25, 0.0], [-1.5, -1.5, -1.5], [0.125, -0.5, -0.375], [3.0, 1.0, -2.0]):
        out.append(pose_at(lo + d))
    for ang in (np.pi / 4, -2.0, 3.0):
        out.append(pose_at(lo + [0.5, 0.25, 0.0], quat((0, 0, 1), ang)))
        out.append(pose_at(lo + [-0.75, -0.5, 0.125], quat((0, 0, 1), ang)))
    out.append(pose_at(lo + [0.625, 0.0, 0.5], quat((1, 2, 3), 0.7)))
    return out


@pytest.mark.parametrize("mesh_name", ["tetra", "cube"])
def test_single_cells_at_the_first_and_last_column_and_level(nav, mesh_name):
    mesh = MESHES[mesh_name]
    c = small_map(nav)
    assert c.set_mesh(*mesh) is True
    assert c.set_boxes(0, ref.cell_centres(CORNER_CELLS, ORIGIN, RES), RES) == 0
    lethal, nonlethal = c.columns(0)
    want = np.zeros((SY, SX), np.uint64)
    for x, y, z in CORNER_CELLS:
        want[y, x] |= np.uint64(1) << np.uint64(z)
    assert np.array_equal(lethal, want) and not nonlethal.any()
    # a mesh half off the extents gives the clipped answer, one wholly off the map the limit and no collision
    poses = [p for cell in CORNER_CELLS for p in poses_around(cell)] + [pose_at(ORIGIN + [-0.5, -0.5, -0.5]), pose_at(ORIGIN + [SX * RES - 0.5, 1.0, 15.75])]
    off = [pose_at([500.0, 500.0, 0.0]), pose_at([-40.0, 1.0, 3.0], quat((0, 0, 1), 1.0))]
    for mode in (ref.DISTANCE, ref.COLLISION_ONLY, ref.COST):
        got, _ = c.query(poses + off, mode=mode)
        assert_costs(got, expected(CORNER_CELLS, ORIGIN, mesh, poses + off, mode))
    got, _ = c.query(poses + off, mode=ref.DISTANCE, distance_limit=1.0)
    assert_costs(got, expected(CORNER_CELLS, ORIGIN, mesh, poses + off, ref.DISTANCE, limit=1.0))
    assert got[-1] == 1.0 and got[-2] == 1.0
    far, _ = c.query(off[:1], mode=ref.DISTANCE)
    assert 100.0 < far[0] < 1000.0  # (no limit: the search grows until it covers the map)
    got, _ = c.query(off, mode=ref.DISTANCE, distance_limit=-1.0)
    assert np.all(got == ref.DBL_MIN)
    c.close()


def test_empty_map_and_limits(nav):
    c = small_map(nav)
    c.set_mesh(*MESHES["cube"])
    poses = [pose_at(ORIGIN + [1.0, 0.5, 1.0])]
    assert c.query(poses, mode=ref.DISTANCE)[0][0] == ref.DBL_MAX
    assert c.query(poses, mode=ref.DISTANCE, distance_limit=2.5)[0][0] == 2.5
    assert c.query(poses, mode=ref.COST)[0][0] == 0.0
    c.close()


def test_pruned_leaves_answer_as_their_cells(nav):
    c = small_map(nav, 2)
    c.set_mesh(*MESHES["tetra"])
    leaves = np.array([ORIGIN + [4 * RES + RES, 2 * RES + RES, 10 * RES + RES], ORIGIN + [64 * RES + 2 * RES, 4 * RES + 2 * RES, 60 * RES + 2 * RES]])
    sizes = np.array([2 * RES, 4 * RES])
    assert c.set_boxes(0, leaves, sizes) == 0
    cells = ref.boxes_to_cells(leaves, sizes, ORIGIN, RES)
    assert len(cells) == 8 + 64
    assert c.set_boxes(1, ref.cell_centres(cells, ORIGIN, RES), RES) == 0
    a, b = c.columns(0), c.columns(1)
    assert a[0].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    poses = poses_around((4, 2, 10)) + poses_around((64, 4, 60))
    got, _ = c.query(poses + poses, runs=[(0, 0, len(poses)), (1, len(poses), len(poses))], mode=ref.DISTANCE)
    assert np.array_equal(got[:len(poses)], got[len(poses):])
    assert_costs(got[:len(poses)], expected(cells, ORIGIN, MESHES["tetra"], poses, ref.DISTANCE))
    c.close()


def test_mark_clear_replace_and_clipped_cells(nav):
    c = small_map(nav)
    rng = np.random.default_rng(5)
    lethal = rng.integers(0, 1 << 62, (SY, SX), dtype=np.uint64) & rng.integers(0, 1 << 62, (SY, SX), dtype=np.uint64)
    nonlethal = rng.integers(0, 1 << 62, (SY, SX), dtype=np.uint64) & ~lethal
    lethal[0, 0] |= np.uint64(1) << np.uint64(63)
    c.set_columns(0, lethal, nonlethal)
    got = c.columns(0)
    assert np.array_equal(got[0], lethal) and np.array_equal(got[1], nonlethal)
    # MARK cells that are free in both planes, then CLEAR them: the planes are back
    free = [(x, y, z) for x, y, z in zip(rng.integers(0, SX, 200), rng.integers(0, SY, 200), rng.integers(0, SZ, 200))
            if not ((int(lethal[y, x]) | int(nonlethal[y, x])) >> int(z)) & 1]
    free = sorted(set(free))
    classes = np.arange(len(free)) % 2
    assert c.set_boxes(0, ref.cell_centres(free, ORIGIN, RES), RES, classes, mode=nav._lib.C3D_MARK) == 0
    marked = c.columns(0)
    want = [lethal.copy(), nonlethal.copy()]
    for (x, y, z), cls in zip(free, classes):
        want[cls][y, x] |= np.uint64(1) << np.uint64(z)
    assert np.array_equal(marked[0], want[0]) and np.array_equal(marked[1], want[1])
    assert c.set_boxes(0, ref.cell_centres(free, ORIGIN, RES), RES, mode=nav._lib.C3D_CLEAR) == 0
    got = c.columns(0)
    assert np.array_equal(got[0], lethal) and np.array_equal(got[1], nonlethal)
    # MARK moves a cell from one class to the other
    x, y, z = free[0]
    c.set_boxes(0, ref.cell_centres([free[0]], ORIGIN, RES), RES, [1], mode=nav._lib.C3D_MARK)
    c.set_boxes(0, ref.cell_centres([free[0]], ORIGIN, RES), RES, [0], mode=nav._lib.C3D_MARK)
    got = c.columns(0)
    assert (int(got[0][y, x]) >> z) & 1 and not (int(got[1][y, x]) >> z) & 1
    # REPLACE is the whole map; a 4-cell leaf with one corner cell inside drops 63 cells, one beyond the map all 8
    boxes = np.array([ORIGIN + [-3 * RES + 2 * RES, -3 * RES + 2 * RES, -3 * RES + 2 * RES], ORIGIN + [SX * RES + RES, RES, RES], ORIGIN + [1.125, 0.125, 0.125]])
    assert c.set_boxes(0, boxes, [4 * RES, 2 * RES, RES], [0, 0, 1]) == 63 + 8
    got = c.columns(0)
    want = np.zeros((SY, SX), np.uint64)
    want[0, 0] = 1
    assert np.array_equal(got[0], want) and int(got[1][0, 4]) == 1 and int(got[1].astype(bool).sum()) == 1
    c.close()


def test_interior_only_collision_and_the_open_mesh(nav):
    c = small_map(nav)
    cell = (20, 3, 8)  # the cube mesh spans four cells each way around it and one more: the cell touches no face
    lo = ORIGIN + np.asarray(cell) * RES
    poses = [pose_at(lo - [0.25, 0.5, 0.25]), pose_at(lo - [0.375, 0.375, 0.375]), pose_at(lo + [0.625, -0.375, -0.25], quat((0, 0, 1), np.pi / 2))]
    c.set_boxes(0, ref.cell_centres([cell], ORIGIN, RES), RES)
    assert c.set_mesh(*MESHES["cube"]) is True
    for mode in (ref.DISTANCE, ref.COST):
        got, _ = c.query(poses, mode=mode)
        assert np.all(got == -1.0)
        assert_costs(got, expected([cell], ORIGIN, MESHES["cube"], poses, mode))
    open_cube = (ref.CUBE_VERTICES, ref.CUBE_TRIANGLES[2:])  # the face z = 0 removed: a surface
    assert c.set_mesh(*open_cube) is False
    got, _ = c.query(poses, mode=ref.DISTANCE)
    want = expected([cell], ORIGIN, open_cube, poses, ref.DISTANCE)
    assert np.all(want > 0) and np.all(got > 0)
    assert_costs(got, want)
    assert np.all(c.query(poses, mode=ref.COLLISION_ONLY)[0] == 0.0)
    c.close()


def test_regions_and_the_nonlethal_plane(nav):
    c = small_map(nav)
    mesh = MESHES["tetra"]
    c.set_mesh(*mesh)
    at = ORIGIN + [5.0, 0.75, 4.0]  # a cell corner: the planes y = at.y, x = at.x lie on cell faces
    base = np.rint((at - ORIGIN) / RES).astype(int)
    L, R, P = ref.LEFT, ref.RIGHT, ref.RECTANGULAR_PRISM
    scale = (0.0, 1.25, 1.5)
    cases = {
        "beyond_left": (base + [2, -2, 0], {L: False, R: True}),      # wholly at y < 0 of the robot
        "touching_left": (base + [2, -1, 0], {L: True, R: True}),     # its face lies on the plane: boundaries are inclusive
        "inside_left": (base + [6, 2, 1], {L: True, R: False}),
        "behind_prism": (base + [-2, 0, 0], {P: False}),              # x < 0
        "touching_prism_back": (base + [-1, 0, 0], {P: True}),
        "beyond_prism_side": (base + [8, 3, 0], {P: False}),          # y in [0.75, 1.0] against |y| <= 0.625
        "straddling_prism_side": (base + [8, 2, 0], {P: True}),       # y in [0.5, 0.75]
        "touching_prism_top": (base + [8, 0, 3], {P: True}),          # z in [0.75, 1.0] against |z| <= 0.75
        "beyond_prism_top": (base + [8, 0, 4], {P: False}),
    }
    pose = pose_at(at)
    for name, (cell, counted) in cases.items():
        c.set_boxes(0, ref.cell_centres([cell], ORIGIN, RES), RES)
        for region, is_counted in counted.items():
            got, _ = c.query([pose], mode=ref.DISTANCE, regions=[region], region_scale=scale)
            want = expected([cell], ORIGIN, mesh, [pose], ref.DISTANCE, regions=[region], scale=scale)
            assert_costs(got, want)
            assert (got[0] < ref.DBL_MAX) == is_counted, (name, region, got)
    # rotated poses, several cells, every region in one call
    cells = [tuple(base + d) for d in ([3, 3, 0], [3, -3, 1], [-3, 1, 0], [5, 0, 2], [0, 4, -3], [1, -1, 0])]
    c.set_boxes(0, ref.cell_centres(cells, ORIGIN, RES), RES)
    poses, regions = [], []
    for q in (quat((0, 0, 1), 0.6), quat((0, 0, 1), -2.5), quat((1, 1, 0), 0.4)):
        for region in (ref.ALL, L, R, P):
            poses.append(pose_at(at + [0.0625, 0.03125, 0.0], q))
            regions.append(region)
    for mode in (ref.DISTANCE, ref.COLLISION_ONLY):
        got, _ = c.query(poses, mode=mode, regions=regions, region_scale=scale)
        assert_costs(got, expected(cells, ORIGIN, mesh, poses, mode, regions=regions, scale=scale))
    # a NONLETHAL cell in the robot: seen in distance mode with obstacles = 1 only
    inside = tuple(base)
    c.set_boxes(0, ref.cell_centres([inside], ORIGIN, RES), RES, [1])
    assert c.query([pose], mode=ref.COST)[0][0] == 0.0
    assert c.query([pose], mode=ref.COLLISION_ONLY, obstacles=[1])[0][0] == 0.0
    assert c.query([pose], mode=ref.DISTANCE)[0][0] == ref.DBL_MAX
    assert c.query([pose], mode=ref.DISTANCE, obstacles=[0])[0][0] == ref.DBL_MAX
    assert c.query([pose], mode=ref.DISTANCE, obstacles=[1])[0][0] == -1.0
    away = pose_at(at + [1.0, 0.0, 0.0])
    got, _ = c.query([away], mode=ref.DISTANCE, obstacles=[1])
    assert_costs(got, expected([inside], ORIGIN, mesh, [away], ref.DISTANCE))
    c.close()


def test_aisles_with_the_robot(nav):
    from navigation_amd.costmap3d import load_stl, read_octomap_bt
    g = np.load(os.path.join(GOLDEN, "c3d_reference.npz"))
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    lo = (t["centres"] - 0.5 * t["sizes"][:, None]).min(0)
    c = nav.Costmap3D(1, 162, 132, 41, t["res"], max_triangles=32, max_boxes=16384, max_poses=64)
    c.set_origin(0, lo)
    assert c.set_boxes(0, t["centres"], t["sizes"], t["classes"]) == 0
    assert sum(bin(int(w)).count("1") for w in c.columns(0)[0].ravel()) == 33 * 8 + 10421
    assert c.set_mesh(*load_stl(os.path.join(GOLDEN, "test_robot.stl"))) is True
    got, results = c.query(g["poses"], mode=ref.DISTANCE)
    want, decided = g["cost"], g["decided"]
    assert (~decided).sum() <= 2
    assert np.array_equal(got[decided] < 0, want[decided] < 0)
    free = decided & (want >= 0)
    print("largest distance difference", np.abs(got[free] - want[free]).max())
    assert np.all(np.abs(got[free] - want[free]) <= TOL)
    assert results["n_lethal"][0] == (got < 0).sum() and results["cost"][0] == -1.0
    collides, _ = c.query(g["poses"], mode=ref.COLLISION_ONLY)
    assert np.array_equal(collides[decided], np.where(want[decided] < 0, -1.0, 0.0))
    c.close()


def test_runs_fold_lazy_and_footprint_costs(nav):
    c = small_map(nav, 3)
    mesh = MESHES["cube"]
    c.set_mesh(*mesh)
    origins = [ORIGIN, ORIGIN + [10.0, -3.0, 0.25], ORIGIN + [-7.5, 2.0, 0.0]]
    maps = [[(10, 3, 2), (14, 3, 2), (30, 1, 3)], [(12, 4, 1), (40, 2, 2)], [(8, 2, 3), (9, 2, 3), (11, 6, 2), (50, 3, 2)]]
    for i in range(3):
        c.set_origin(i, origins[i])
        assert np.array_equal(c.origin(i), origins[i])
        c.set_boxes(i, ref.cell_centres(maps[i], origins[i], RES), RES)
    rng = np.random.default_rng(11)

    def path(i, n):  # a walk along x through the map's cells at their height
        x = origins[i][0] + np.linspace(0.0, 14.0, n)
        return [[x[k], origins[i][1] + 0.25 + 0.5 * rng.random(), 0.0, rng.uniform(-np.pi, np.pi)] for k in range(n)]

    runs_of = [2, 0, 1, 0]  # shuffled, instance 0 twice
    xyth, runs = [], []
    for i in runs_of:
        p = path(i, 9)
        runs.append((i, len(xyth), len(p)))
        xyth += p
    xyth = np.array(xyth)
    poses = np.array([ref.yaw_pose(*p[[0, 1, 3]]) for p in xyth])
    poses[:, 2] = 0.25  # (the yaw poses lifted off z = 0 for the query; footprint_costs below stays on it)
    for mode in (ref.DISTANCE, ref.COLLISION_ONLY, ref.COST):
        want = np.concatenate([expected(maps[i], origins[i], mesh, poses[f:f + n], mode, limit=3.0) for i, f, n in runs])
        got, results = c.query(poses, runs=runs, mode=mode, distance_limit=3.0)
        assert_costs(got, want)
        assert (want < 0).any() and (want >= 0).any()
        for lazy in (False, True):
            sentinel = np.full(len(poses), 12345.0)
            got, results = c.query(poses, runs=runs, mode=mode, distance_limit=3.0, lazy=lazy, pose_costs=sentinel)
            for k, (i, f, n) in enumerate(runs):
                w = ref.fold(want[f:f + n], mode, lazy)
                r = results[k]
                assert (r["n_lethal"], r["first_lethal"], r["n_done"]) == (w["n_lethal"], w["first_lethal"], w["n_done"]), (mode, lazy, k)
                assert abs(r["cost"] - w["cost"]) <= TOL
                assert np.all(got[f + r["n_done"]:f + n] == 12345.0)
                assert_costs(got[f:f + r["n_done"]], want[f:f + r["n_done"]])
            if lazy:
                assert any(results[k]["n_done"] < runs[k][2] for k in range(len(runs)))
    # Costmap3DModel::footprintCost: (x, y, 0) with the yaw quaternion, the cost mode over ALL
    flat = np.array([ref.yaw_pose(*p[[0, 1, 3]]) for p in xyth])
    costs, first = c.footprint_costs(xyth[:, [0, 1, 3]], runs=runs)
    got, results = c.query(flat, runs=runs, mode=ref.COST)
    assert np.array_equal(costs, got) and np.array_equal(first, results["first_lethal"])
    assert_costs(costs, np.concatenate([expected(maps[i], origins[i], mesh, flat[f:f + n], ref.COST) for i, f, n in runs]))
    # a query runs behind the set_boxes queued just before it
    probe = [pose_at(origins[1] + [6.0, 1.0, 0.25])]
    before, _ = c.query(probe, runs=[(1, 0, 1)], mode=ref.COLLISION_ONLY)
    c.set_boxes(1, ref.cell_centres([(25, 5, 2)], origins[1], RES), RES, mode=nav._lib.C3D_MARK)
    after, _ = c.query(probe, runs=[(1, 0, 1)], mode=ref.COLLISION_ONLY)
    assert before[0] == 0.0 and after[0] == -1.0
    c.close()


def test_errors_change_nothing_resident(nav):
    c = small_map(nav)
    c.set_mesh(*MESHES["tetra"])
    cells = [(3, 3, 3), (40, 2, 63)]
    c.set_boxes(0, ref.cell_centres(cells, ORIGIN, RES), RES)
    poses = poses_around((3, 3, 3))
    columns = c.columns(0)
    answers, _ = c.query(poses, mode=ref.DISTANCE)

    def unchanged():
        now = c.columns(0)
        assert np.array_equal(now[0], columns[0]) and np.array_equal(now[1], columns[1])
        assert np.array_equal(c.query(poses, mode=ref.DISTANCE)[0], answers)

    with pytest.raises(nav.NavgpuError, match=r"\(-4\)"):
        c.set_boxes(0, np.tile(ORIGIN + 0.125, (257, 1)), RES)  # max_boxes is 256
    with pytest.raises(nav.NavgpuError, match=r"\(-1\)"):
        c.set_boxes(0, [ORIGIN + 0.125, ORIGIN + [0.125, 0.2, 0.125]], RES)  # the second is not on the grid
    with pytest.raises(nav.NavgpuError, match=r"\(-1\)"):
        c.set_boxes(0, [ORIGIN + 0.375], 3 * RES)  # not resolution * 2^k
    unchanged()
    big_v = np.concatenate([ref.CUBE_VERTICES, ref.CUBE_VERTICES + 2.0])
    big_t = np.concatenate([ref.CUBE_TRIANGLES, ref.CUBE_TRIANGLES + 8])
    with pytest.raises(nav.NavgpuError, match=r"\(-4\)"):
        c.set_mesh(big_v, big_t)  # 24 triangles, max_triangles is 16
    with pytest.raises(nav.NavgpuError, match=r"\(-1\)"):
        c.set_mesh(ref.TETRA_VERTICES, [[0, 1, 1]])  # no area
    unchanged()
    with pytest.raises(nav.NavgpuError, match=r"\(-1\)"):
        c.query(poses, mode=3)
    with pytest.raises(nav.NavgpuError, match=r"\(-1\)"):
        c.query([pose_at(ORIGIN, (0.0, 0.0, 0.0, 0.0))], mode=ref.COST)
    with pytest.raises(nav.NavgpuError, match=r"\(-4\)"):
        c.query(np.tile(pose_at(ORIGIN), (257, 1)), mode=ref.COST)  # max_poses is 256
    with pytest.raises(nav.NavgpuError, match=r"\(-1\)"):
        c.query(poses, runs=[(0, 0, 3), (0, 2, 2)], mode=ref.COST)  # the runs share pose 2
    unchanged()
    c.close()
