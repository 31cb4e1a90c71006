"""CPU checks of the costmap_3d yardstick (tests/costmap3d_ref.py) and of the two file readers: the fixtures parse to the counts
the reference's files have, closed-form separations come out of the yardstick, and it reproduces tests/golden/costmap3d/c3d_reference.npz
(tools/make_costmap3d_goldens.py), the file the GPU test reads."""
import os
import sys

import numpy as np
import pytest

import costmap3d_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")
CUBE = (ref.CUBE_VERTICES, ref.CUBE_TRIANGLES)
OPEN_CUBE = (ref.CUBE_VERTICES, ref.CUBE_TRIANGLES[2:])  # the face z = 0 removed


@pytest.fixture(scope="module")
def aisles():
    from navigation_amd.costmap3d import read_octomap_bt
    return read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))


@pytest.fixture(scope="module")
def robot():
    from navigation_amd.costmap3d import load_stl
    return load_stl(os.path.join(GOLDEN, "test_robot.stl"))


def test_bt_reader_reproduces_the_tree(aisles):
    from navigation_amd.costmap3d import load_octomap_bt
    t = aisles
    assert (t["res"], t["depth"], t["size"], t["n_nodes"]) == (0.05, 24, 17925, 17925)
    assert len(t["sizes"]) == 10454 and np.all(t["classes"] == 0)
    assert np.array_equal(np.bincount(t["depths"], minlength=25)[[23, 24]], [33, 10421]) and t["depths"].min() == 23
    lo = (t["centres"] - 0.5 * t["sizes"][:, None]).min(0)
    hi = (t["centres"] + 0.5 * t["sizes"][:, None]).max(0)
    assert np.allclose(lo, [-39.25, 21.85, 0.05], atol=1e-9) and np.allclose(hi, [-31.15, 28.45, 2.10], atol=1e-9)
    assert np.array_equal(np.rint((hi - lo) / t["res"]), [162, 132, 41])
    cells = ref.boxes_to_cells(t["centres"], t["sizes"], lo, t["res"])
    assert len(cells) == len(np.unique(cells, axis=0)) == 33 * 8 + 10421
    centres, sizes, classes = load_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    assert np.array_equal(centres, t["centres"]) and np.array_equal(sizes, t["sizes"]) and np.array_equal(classes, t["classes"])


def test_bt_reader_refuses_a_short_or_long_payload(tmp_path):
    from navigation_amd.costmap3d import read_octomap_bt
    data = open(os.path.join(GOLDEN, "aisles.bt"), "rb").read()
    for name, bad in (("short.bt", data[:-2]), ("long.bt", data + b"\0\0")):
        (tmp_path / name).write_bytes(bad)
        with pytest.raises((AssertionError, ValueError)):
            read_octomap_bt(str(tmp_path / name))


def test_stl_reader(robot):
    vertices, triangles = robot
    assert triangles.shape == (28, 3) and vertices.shape == (16, 3)
    assert ref.mesh_closed(triangles) and not ref.mesh_closed(triangles[1:])
    assert abs(ref.mesh_volume(vertices, triangles) - 0.494) <= 0.001
    assert np.allclose(vertices.min(0), [-0.5, -0.35, 0.0], atol=1e-6) and np.allclose(vertices.max(0), [0.5, 0.35, 2.05], atol=1e-6)


def test_meshes_of_the_tests():
    assert ref.mesh_closed(ref.CUBE_TRIANGLES) and abs(ref.mesh_volume(*CUBE) - 1.0) < 1e-15
    assert ref.mesh_closed(ref.TETRA_TRIANGLES) and abs(ref.mesh_volume(ref.TETRA_VERTICES, ref.TETRA_TRIANGLES) - 1.0 / 6.0) < 1e-15
    assert not ref.mesh_closed(OPEN_CUBE[1])


def one_box(centre, size, pose, mesh=CUBE, **kw):
    return ref.query_pose(np.array([centre], np.float64), size, mesh[0], mesh[1], np.asarray(pose, np.float64), **kw)


IDENTITY = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


def test_face_edge_and_vertex_separations():
    # the unit cube [0, 1]^3 against a box of edge 0.5: gaps g along one, two and three axes
    g = 0.375
    c = 1.0 + g + 0.25
    assert one_box([c, 0.5, 0.5], 0.5, IDENTITY) == pytest.approx(g, abs=1e-15)
    assert one_box([c, c, 0.5], 0.5, IDENTITY) == pytest.approx(g * np.sqrt(2.0), abs=1e-15)
    assert one_box([c, c, c], 0.5, IDENTITY) == pytest.approx(g * np.sqrt(3.0), abs=1e-15)
    assert one_box([-g - 0.25, 0.5, -g - 0.25], 0.5, IDENTITY) == pytest.approx(g * np.sqrt(2.0), abs=1e-15)
    # touching is collision, in every mode; a hair apart is not
    for mode in (ref.DISTANCE, ref.COST, ref.COLLISION_ONLY):
        assert one_box([1.25, 0.5, 0.5], 0.5, IDENTITY, mode=mode) == -1.0
        assert one_box([1.25, 1.25, 1.25], 0.5, IDENTITY, mode=mode) == -1.0
    assert one_box([1.25 + 2.0 ** -20, 0.5, 0.5], 0.5, IDENTITY) == 2.0 ** -20
    # the limit: a distance at or above it is the limit, DBL_MAX stays DBL_MAX, <= 0 becomes DBL_MIN
    assert one_box([c, 0.5, 0.5], 0.5, IDENTITY, limit=0.25) == 0.25
    assert one_box([c, 0.5, 0.5], 0.5, IDENTITY, limit=0.0) == ref.DBL_MIN
    assert ref.query_pose(np.zeros((0, 3)), 0.5, CUBE[0], CUBE[1], np.array(IDENTITY)) == ref.DBL_MAX


def test_yaw_of_45_degrees():
    # the cube turned by 45 degrees about z at the origin: the corner (1, 0) goes to (r, r), r = sqrt 1/2, the edge to it lies on y = x
    pose = ref.yaw_pose(0.0, 0.0, np.pi / 4)
    r = np.sqrt(0.5)
    # a box to the right of the turned square's right corner (r, r): gap along x
    assert one_box([r + 0.5 + 0.25, r, 0.5], 0.5, pose) == pytest.approx(0.5, abs=1e-12)
    # a box below the edge from (0, 0) to (r, r), its corner (x0, y0) nearest: distance |x0 - y0| / sqrt 2
    x0, y0 = 1.0, 0.25  # the box's upper left corner
    d = one_box([x0 + 0.25, y0 - 0.25, 0.5], 0.5, pose)
    # (the nearest point of the square to that corner is on the edge when its foot (x0 + y0) / 2 * (1, 1) lies within it)
    assert (x0 + y0) / 2 <= r and d == pytest.approx((x0 - y0) / np.sqrt(2.0), abs=1e-12)


def test_interior_only_collision_and_the_open_mesh():
    # a box of edge 0.25 wholly inside the cube, touching no face: the interior test alone finds it
    centre = [0.5, 0.375, 0.625]
    V = ref.world_triangles(CUBE[0], CUBE[1], np.array(IDENTITY))[None] - np.array(centre)[None, None, None, :]
    assert not ref.overlap(V, 0.125).any()
    assert abs(abs(ref.winding(np.array([centre]), ref.world_triangles(*CUBE, np.array(IDENTITY)))[0]) - 1.0) < 1e-12
    assert abs(ref.winding(np.array([[1.5, 0.5, 0.5]]), ref.world_triangles(*CUBE, np.array(IDENTITY)))[0]) < 1e-12
    for mode in (ref.DISTANCE, ref.COST, ref.COLLISION_ONLY):
        assert one_box(centre, 0.25, IDENTITY, mode=mode) == -1.0
    # the same box against the open mesh: a surface has no inside
    assert one_box(centre, 0.25, IDENTITY, mesh=OPEN_CUBE, mode=ref.COST) == 0.0
    assert one_box(centre, 0.25, IDENTITY, mesh=OPEN_CUBE) == pytest.approx(0.25, abs=1e-15)  # to the face y = 0


def test_regions():
    pose = [2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    left, right = [2.5, 3.0 + 1.75, 0.5], [2.5, 3.0 - 0.75, 0.5]  # boxes of edge 0.5 wholly on one side of y = 3
    for box, region, seen in ((left, ref.LEFT, True), (left, ref.RIGHT, False), (right, ref.RIGHT, True), (right, ref.LEFT, False)):
        assert (one_box(box, 0.5, pose, region=region) < ref.DBL_MAX) == seen
    touching = [2.5, 3.0 - 0.25, 0.5]  # its face lies on the plane: counted by both (and it touches the cube)
    assert one_box(touching, 0.5, pose, region=ref.LEFT) == -1.0 and one_box(touching, 0.5, pose, region=ref.RIGHT) == -1.0
    scale = (0.0, 3.0, 1.0)  # the prism: x >= 0, |y| <= 1.5, |z| <= 0.5 about the pose
    assert one_box([2.0 - 0.75, 3.0, 0.0], 0.5, pose, region=ref.RECTANGULAR_PRISM, scale=scale) == ref.DBL_MAX
    assert one_box([2.0 - 0.25, 3.0 - 1.0, 0.0], 0.5, pose, region=ref.RECTANGULAR_PRISM, scale=scale) < ref.DBL_MAX
    assert one_box([4.0, 3.0 + 1.75, 0.0], 0.5, pose, region=ref.RECTANGULAR_PRISM, scale=scale) < ref.DBL_MAX   # touches y = 1.5
    assert one_box([4.0, 3.0 + 1.75 + 2.0 ** -30, 0.0], 0.5, pose, region=ref.RECTANGULAR_PRISM, scale=scale) == ref.DBL_MAX
    assert one_box([4.0, 3.0, 1.0], 0.5, pose, region=ref.RECTANGULAR_PRISM, scale=scale) == ref.DBL_MAX  # z in [0.75, 1.25]


def test_fold():
    assert ref.fold([0.5, 0.25, 2.0], ref.DISTANCE) == dict(cost=0.25, n_lethal=0, first_lethal=-1, n_done=3)
    assert ref.fold([0.5, -1.0, 2.0, -1.0], ref.DISTANCE) == dict(cost=-1.0, n_lethal=2, first_lethal=1, n_done=4)
    assert ref.fold([], ref.DISTANCE)["cost"] == ref.DBL_MAX
    assert ref.fold([0.0, -1.0, 0.0, -1.0, -1.0], ref.COST) == dict(cost=-3.0, n_lethal=3, first_lethal=1, n_done=5)
    assert ref.fold([0.0, -1.0, 0.0, -1.0], ref.COST, lazy=True) == dict(cost=-1.0, n_lethal=1, first_lethal=1, n_done=2)
    assert ref.fold([0.0, 0.0], ref.COLLISION_ONLY, lazy=True) == dict(cost=0.0, n_lethal=0, first_lethal=-1, n_done=2)


def test_pad_points_is_the_reference_arithmetic_in_float():
    v = np.array([[0.0, 0.0, 1.0], [3.0, 4.0, 0.5], [-0.5, 0.35, 2.0]])
    p = ref.pad_points(v, 0.1)
    assert np.array_equal(p[0], v[0]) and np.array_equal(p[:, 2], v[:, 2])
    assert np.allclose(np.hypot(p[1:, 0], p[1:, 1]), np.hypot(v[1:, 0], v[1:, 1]) + 0.1, atol=1e-6)
    assert np.array_equal(p[1:, :2], p[1:, :2].astype(np.float32))  # float results
    assert np.array_equal(ref.pad_points(v, 0.0), v)


def test_the_yardstick_reproduces_the_golden_file(aisles, robot):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_costmap3d_goldens as tool
    g = np.load(os.path.join(GOLDEN, "c3d_reference.npz"))
    origin, size, res, cells, _ = tool.aisles()
    assert tuple(size) == (162, 132, 41)
    poses = tool.poses_of(int(g["seed"]), origin, origin + size * res)
    assert np.array_equal(poses, g["poses"]) and poses.shape == (48, 7)
    assert np.all(np.abs(poses[:40, 3:5]) == 0) and np.all(np.abs(poses[40:, 3:5]).max(1) > 0.03)  # 8 poses with a roll or a pitch
    cost, verdict, decided = tool.answers(poses, ref.cell_centres(cells, origin, res), res, *robot)
    assert np.array_equal(cost, g["cost"]) and np.array_equal(verdict, g["verdict"]) and np.array_equal(decided, g["decided"])
    assert decided.all()  # the seed leaves no borderline pose
    assert 10 <= (cost < 0).sum() <= 38
