"""Closed forms that hold the rolling yardstick (tests/costmap3d_rolling_ref.py) in place: what it is compared with must itself say
what include/navgpu_costmap3d_rolling.h says.  Everything is integers, bytes, or doubles from expressions written out here, so
every comparison is equality."""
import numpy as np

import costmap3d_layers_ref as ref
import costmap3d_rolling_ref as roll

RES = 0.25
ORIGIN = np.array([-2.0, 1.0, -0.5])
SIZE = (72, 8, 64)
CLOUD = dict(kind=ref.POINT_CLOUD)
STATIC = dict(kind=ref.STATIC_2D, height=-0.5, lethal_cost_threshold=100, unknown_to_lethal=0)
CYLINDER = dict(kind=ref.CYLINDER_CLEARING, radius=0.8)


def centre_of(cell, origin=ORIGIN):
    return np.asarray(origin) + (np.asarray(cell) + 0.5) * RES


def fresh(layers=(CLOUD,), origin=ORIGIN, size=SIZE):
    m = roll.RollingMap(size, origin, RES, list(layers))
    m.update((0.0, 0.0, 0.0))  # the first, full update
    return m


def state(m):
    return [m.master.copy(), m.layer2d.copy()] + [v.copy() for v in m.vol if v is not None] + [c.copy() for c in m.changed if c is not None]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_cell_stays_at_its_world_position_and_leaves_for_good():
    m = fresh()
    world = centre_of((10, 3, 5))
    m.buffer_cloud(0, [world])
    m.update((0.0, 0.0, 0.0))
    assert m.master[10, 3, 5] == ref.LETHAL and (m.master != ref.ABSENT).sum() == 1
    origin_x, left = ORIGIN[0], False
    for step, present in ((3, True), (4, True), (3, True), (1, False), (-11, False)):  # keys -8 -> -5 -> -1 -> 2 -> 3 -> -8
        origin_x += step * RES
        assert m.roll_origin((origin_x, ORIGIN[1])) == (step, 0)
        cell, finite = ref.coord_to_cell(world, RES, ref.origin_keys(m.origin, RES))
        assert finite.all()
        left = left or not 0 <= cell[0] < SIZE[0]
        assert present == (not left)
        for vol in (m.master, m.vol[0]):
            assert (vol != ref.ABSENT).sum() == (1 if present else 0)
            if present:
                assert vol[cell[0], cell[1], cell[2]] == ref.LETHAL
        assert (m.layer2d == 254).sum() == (1 if present else 0)
        if present:
            assert m.layer2d[cell[1], cell[0]] == 254
    # the window is back where it began and the column that left is empty: it does not return
    assert np.array_equal(m.origin, ORIGIN) and not m.master.any() and not m.vol[0].any() and (m.layer2d == 255).all()


def test_the_cell_vanishes_exactly_when_its_column_leaves():
    for axis, cell in ((0, (2, 3, 0)), (1, (40, 2, 63))):
        m = fresh()
        m.buffer_cloud(0, [centre_of(cell)])
        m.update((0.0, 0.0, 0.0))
        for k in range(1, 4):
            target = ORIGIN[:2].copy()
            target[axis] += k * RES
            m.roll_origin(target)
            assert bool(m.master.any()) == (k <= 2) and bool(m.vol[0].any()) == (k <= 2)
    m = fresh()  # and at the other edge, rolling down
    m.buffer_cloud(0, [centre_of((70, 3, 0))])
    m.update((0.0, 0.0, 0.0))
    assert m.roll_origin((ORIGIN[0] - RES, ORIGIN[1])) == (-1, 0) and m.master[71, 3, 0] == ref.LETHAL
    assert m.roll_origin((ORIGIN[0] - 2 * RES, ORIGIN[1])) == (-1, 0) and not m.master.any()


def test_two_rolls_equal_their_sum_when_nothing_leaves_between():
    rng = np.random.default_rng(1)
    pts = (ORIGIN + np.array([20, 3, 0]) * RES + rng.random((200, 3)) * np.array([30, 2, 60]) * RES).astype(np.float32)  # columns 20..49, rows 3..4
    a, b = fresh(), fresh()
    for m in (a, b):
        m.buffer_cloud(0, pts)
        m.update((0.0, 0.0, 0.0))
        m.buffer_cloud(0, pts[:120])  # pending changed bits
    assert a.roll_origin(ORIGIN[:2] + np.array([5, -2]) * RES) == (5, -2)
    assert a.roll_origin(ORIGIN[:2] + np.array([-7, 1]) * RES) == (-12, 3)
    assert b.roll_origin(ORIGIN[:2] + np.array([-7, 1]) * RES) == (-7, 1)
    assert a.master.any() and a.changed[0].any() and same(state(a), state(b)) and np.array_equal(a.origin, b.origin)


def test_a_rolled_map_equals_a_fresh_one_given_the_cropped_content():
    rng = np.random.default_rng(2)
    hi = ORIGIN + np.array(SIZE) * RES
    pts = (ORIGIN + rng.random((600, 3)) * (hi - ORIGIN)).astype(np.float32)
    m = fresh()
    m.buffer_cloud(0, pts)
    m.update((0.0, 0.0, 0.0))
    new_origin = ORIGIN + np.array([9, -3, 0]) * RES
    assert m.roll_origin(new_origin[:2]) == (9, -3)
    # the content that survives: the points whose cell lies inside both windows
    cells, _ = ref.coord_to_cell(pts.astype(np.float64), RES, ref.origin_keys(ORIGIN, RES))
    in_old = np.all((cells >= 0) & (cells < np.array(SIZE)), axis=1)
    f = fresh(origin=new_origin)
    f.buffer_cloud(0, pts[in_old])
    f.update((0.0, 0.0, 0.0))
    assert f.master.any() and np.array_equal(m.master, f.master) and np.array_equal(m.vol[0], f.vol[0]) and np.array_equal(m.layer2d, f.layer2d)
    assert np.array_equal(m.origin, f.origin)


def test_the_float_rule_of_the_centre_mode():
    size_x = 72
    boundary = 1.25  # a cell face: key 5 at 0.25 m
    x = np.float64(boundary + 9.0) - np.float64(1e-9)
    lower = x - np.float64(size_x * RES) / 2.0
    assert lower < boundary and boundary - lower < np.spacing(np.float32(boundary)) / 2  # below the face by less than half a float ulp
    assert int(np.floor(lower * (1.0 / RES))) == 4        # in double the robot's window starts a cell lower
    assert np.float32(lower) == np.float32(boundary)      # the float of octomap::point3d lands on the face
    assert int(np.floor(np.float64(np.float32(lower)) * (1.0 / RES))) == 5
    assert roll.centre_key(x, size_x, RES) == 5
    m = fresh()
    assert m.roll_centre((x, 2.0)) == (5 - (-8), int(np.floor((2.0 - 1.0) * 4)) - 4)
    assert m.origin[0] == 5 * RES and m.origin[1] == 1.0 and m.origin[2] == ORIGIN[2]
    # an ordinary pose: the window's lower corner is the robot less half the extent, floored to the lattice
    assert roll.centre_key(0.3, 72, RES) == int(np.floor((0.3 - 9.0) * 4)) == -35 and roll.centre_key(-0.3, 8, RES) == -6


def test_z_never_rolls():
    m = fresh(origin=ORIGIN + np.array([0.0, 0.0, 0.75]))
    m.roll_centre((100.0, -30.0))
    m.roll_origin((3.0, 4.0))
    assert m.origin[2] == ORIGIN[2] + 0.75 and tuple(m.origin[:2]) == (3.0, 4.0)


def test_update_reports_the_whole_window_once_after_a_roll():
    m = fresh()
    assert m.update((0.0, 0.0, 0.0)) == ref.EMPTY_BOUNDS
    assert m.roll_origin(ORIGIN[:2]) == (0, 0) and m.update((0.0, 0.0, 0.0)) == ref.EMPTY_BOUNDS  # a shift of (0, 0) is no move
    m.roll_origin((-1.0, 1.5))
    assert m.update((0.0, 0.0, 0.0)) == (-1.0, 1.5, -1.0 + 72 * RES, 1.5 + 8 * RES)
    assert m.update((0.0, 0.0, 0.0)) == ref.EMPTY_BOUNDS
    m.roll_origin((-1.25, 1.5))
    m.reset()  # the full flag implies the mark: the bounds are the window either way
    assert m.update((0.0, 0.0, 0.0)) == (-1.25, 1.5, -1.25 + 72 * RES, 1.5 + 8 * RES) and m.update((0.0, 0.0, 0.0)) == ref.EMPTY_BOUNDS


def test_a_roll_beyond_the_size_empties_everything():
    m = fresh()
    m.buffer_cloud(0, [centre_of((10, 3, 5)), centre_of((71, 7, 63))])
    assert m.roll_origin((ORIGIN[0], ORIGIN[1] + 8 * RES)) == (0, 8)
    assert not m.vol[0].any() and not m.changed[0].any() and not m.master.any() and not m.full


def filled(layers):
    m = fresh(layers)
    grid = np.full((SIZE[1], SIZE[0]), 100, np.int8)
    hi = ORIGIN + np.array(SIZE) * RES
    pts = (ORIGIN + np.random.default_rng(3).random((3000, 3)) * (hi - ORIGIN)).astype(np.float32)
    for k, l in enumerate(layers):
        if l["kind"] == ref.STATIC_2D:
            m.set_static_grid(k, grid, ORIGIN[0], ORIGIN[1])
        elif l["kind"] == ref.POINT_CLOUD:
            m.buffer_cloud(k, pts)
    m.update((0.0, 0.0, 0.0))
    return m


def test_reset_bounding_box():
    layers = (STATIC, CLOUD, CYLINDER)
    m = filled(layers)
    before = m.vol[1].copy()
    static_before, master_before = m.vol[0].copy(), m.master.copy()
    # clipped by the window on two sides: x from below the window to the middle of column 65, y from row 6 to beyond, levels 2..9
    box = (ORIGIN[0] - 3.0, ORIGIN[1] + 6 * RES, ORIGIN[2] + 2 * RES, ORIGIN[0] + 65.5 * RES, ORIGIN[1] + 40.0, ORIGIN[2] + 9.99 * RES)
    m.reset_bounding_box(box, (0, 1, 2))
    region = np.zeros(SIZE, bool)
    region[0:66, 6:8, 2:10] = True
    assert (before[region] != ref.ABSENT).sum() > 20
    assert not m.vol[1][region].any() and np.array_equal(m.vol[1][~region], before[~region])        # deleted inside, and nowhere else
    assert np.array_equal(m.changed[1], region & (before != ref.ABSENT))                              # the deleted cells, and nothing else
    assert np.array_equal(m.vol[0], static_before) and not m.changed[0].any()                         # a STATIC_2D layer ignores the call
    assert np.array_equal(m.master, master_before)                                                    # until the next update
    m.update((0.0, 0.0, 0.0))
    assert not m.master[region].any() and m.master[:, :, 0].all() and not m.changed[1].any()         # (the static floor is level 0)
    # both ends are inclusive: a box of one point deletes that point's cell
    m = filled((CLOUD,))
    p = centre_of((64, 0, 63))
    m.vol[0][64, 0, 63] = ref.LETHAL
    count = (m.vol[0] != ref.ABSENT).sum()
    m.reset_bounding_box(tuple(p) + tuple(p), (0,))
    assert (m.vol[0] != ref.ABSENT).sum() == count - 1 and m.changed[0].sum() == 1 and m.changed[0][64, 0, 63]


def test_reset_bounding_box_that_deletes_nothing():
    m = filled((CLOUD,))
    before = state(m)
    hi = ORIGIN + np.array(SIZE) * RES
    m.reset_bounding_box((hi[0] + 0.01, ORIGIN[1], ORIGIN[2], hi[0] + 5.0, hi[1], hi[2]), (0,))       # wholly outside, beyond the maximum
    m.reset_bounding_box((ORIGIN[0] - 5.0, ORIGIN[1], ORIGIN[2], ORIGIN[0] - 0.01, hi[1], hi[2]), (0,))  # and below the minimum
    for a in range(3):                                                                                # min > max on one axis
        box = list(ORIGIN) + list(hi)
        box[a], box[3 + a] = box[3 + a], box[a]
        m.reset_bounding_box(tuple(box), (0,))
    m.reset_bounding_box(tuple(ORIGIN) + tuple(hi), ())                                               # no layer named
    assert same(before, state(m))
    m.reset_bounding_box(tuple(ORIGIN) + tuple(hi), (0,))                                             # and the whole window
    assert not m.vol[0].any() and np.array_equal(m.changed[0], before[2] != ref.ABSENT)
