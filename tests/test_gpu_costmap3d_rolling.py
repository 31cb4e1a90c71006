"""Rolling 3-D maps and resetBoundingBox on the device (include/navgpu_costmap3d_rolling.h) against the numpy yardstick
(tests/costmap3d_rolling_ref.py): the same grids, clouds, poses, rolls and boxes on both sides.

Everything the feature computes is integers, bits, bytes, or doubles from expressions both sides evaluate alike, so every comparison
is equality: after each step the master's three planes, each costmap layer's planes and `changed` plane, the 2-D bytes and the
origin.  (The one distance query also keeps the query's own 1e-9 m bound against tests/costmap3d_ref.py, beside an exact comparison
with a fresh handle that is given the yardstick's planes.)  The maps are 72 x 8 x 64 cells of 0.25 m at origin (-2, 1, -0.5): two
tiles per row, the second with 8 live columns, and bit 63 in use.  The stack is static floor + xyzi cloud + cylinder.

The content is hand-placed: the static layer has cells in columns 0, 63, 64, 71 of rows 0 and 7; the cloud layer has cells of all
three classes at levels 0 and 63 in those columns of row 0 but only in columns 64 and 71 of row 7 and in rows 3 and 4 otherwise - so
rows 1, 2, 5, 6 and the first tile of row 7 are empty tiles there, and a roll moves cells into tiles that were empty before: the
case that fails at the next buffer_clouds / update when an occupancy or dirty bit is stale."""
import copy

import numpy as np
import pytest

import costmap3d_layers_ref as ref
import costmap3d_ref as qref
import costmap3d_rolling_ref as roll

pytestmark = pytest.mark.gpu

RES = 0.25
ORIGIN = np.array([-2.0, 1.0, -0.5])
SX, SY, SZ = 72, 8, 64
SIZE = (SX, SY, SZ)
XYZI = dict(kind=ref.POINT_CLOUD, cloud_has_intensity=1, free_intensity=0.25, lethal_intensity=0.75)
STATIC = dict(kind=ref.STATIC_2D, height=-0.5, lethal_cost_threshold=100, unknown_to_lethal=0)
CYLINDER = dict(kind=ref.CYLINDER_CLEARING, radius=0.8)
STACK = [STATIC, XYZI, CYLINDER]
ROBOT = (6.1, 2.1, 0.0)  # the cylinder clears columns round (32, 4)
INTENSITY = (0.0, 0.5, 1.0)  # FREE, NONLETHAL, LETHAL
FLOAT_RULE_X = np.float64(1.25 + 9.0) - np.float64(1e-9)  # tests/test_costmap3d_rolling_reference.py: the float lands on the face, key 5


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def centre_of(cell, origin=ORIGIN):
    return np.asarray(origin) + (np.asarray(cell) + 0.5) * RES


def points_at(cells, origin=ORIGIN):
    """one xyzi point at the centre of each cell, the classes taking turns"""
    return np.array([list(centre_of(c, origin)) + [INTENSITY[k % 3]] for k, c in enumerate(cells)], np.float32)


def content(instance):
    """(static grid, the cloud an update has consumed, the cloud that is pending) of one instance"""
    rng = np.random.default_rng(100 + instance)
    grid = np.full((SY, SX), -1, np.int8)
    for y in (0, 7):
        for x in (0, 63, 64, 71):
            grid[y, x] = 100
    grid[3:5, 10:60] = rng.choice(np.array([-1, 0, 100], np.int8), (2, 50))
    cells = [(x, 0, z) for x in (0, 63, 64, 71) for z in (0, 63)] + [(x, 7, z) for x in (64, 71) for z in (0, 63)]
    cells += [(int(x), int(y), int(z)) for x, y, z in zip(rng.integers(1, 71, 90), rng.integers(3, 5, 90), rng.integers(0, 64, 90))]
    first = points_at(cells)
    pending = points_at(cells[:9] + cells[12:70] + [(int(x), 4, int(z)) for x, z in zip(rng.integers(60, 70, 12), rng.integers(0, 64, 12))])
    return grid, first, pending


@pytest.fixture(scope="module")
def prototype():
    """the yardstick's maps in the state every case starts from, computed once; a case takes a deep copy"""
    maps = []
    for i in range(3):
        m = roll.RollingMap(SIZE, ORIGIN, RES, STACK)
        grid, first, pending = content(i)
        assert m.set_static_grid(0, grid, ORIGIN[0], ORIGIN[1]) == 0 and m.buffer_cloud(1, first) == 0
        m.update(ROBOT)
        assert m.buffer_cloud(1, pending) == 0
        assert {ref.FREE, ref.NONLETHAL, ref.LETHAL} <= set(np.unique(m.master)) and m.changed[1].any() and not m.vol[1][:, (1, 2, 5, 6)].any()
        assert not m.vol[1][:64, 7].any() and m.vol[1][64:, 7].any()
        maps.append(m)
    return maps


def build(nav, prototype):
    """the device handle in the prototype's state, and a copy of the yardstick's maps"""
    c = nav.Costmap3D(3, SX, SY, SZ, RES, max_triangles=16, max_boxes=256, max_poses=64)
    for i in range(3):
        c.set_origin(i, ORIGIN)
    c.configure_layers([dict(max_cloud_points=4096, **l) for l in STACK])
    for i in range(3):
        grid, first, pending = content(i)
        c.set_static_grid(i, 0, grid, ORIGIN[0], ORIGIN[1])
        c.buffer_clouds([(i, 1, 0, len(first))], first)
    c.update([0, 1, 2], [ROBOT] * 3)
    pend = [content(i)[2] for i in range(3)]
    starts = np.cumsum([0] + [len(p) for p in pend])
    c.buffer_clouds([(i, 1, int(starts[i]), len(pend[i])) for i in range(3)], np.concatenate(pend))
    return c, copy.deepcopy(prototype)


def assert_equal_state(c, m, instance=0):
    """the master's three planes, every costmap layer's planes and changed plane, the 2-D layer and the origin"""
    lethal, nonlethal = c.columns(instance)
    assert np.array_equal(lethal, ref.to_words(m.master, ref.LETHAL)), "master LETHAL"
    assert np.array_equal(nonlethal, ref.to_words(m.master, ref.NONLETHAL)), "master NONLETHAL"
    assert np.array_equal(c.free_columns(instance), ref.to_words(m.master, ref.FREE)), "master FREE"
    for k, l in enumerate(m.layers):
        if l["kind"] == ref.CYLINDER_CLEARING:
            continue
        got = c.layer_columns(instance, k)
        for plane, state in zip(got[:3], (ref.LETHAL, ref.NONLETHAL, ref.FREE)):
            assert np.array_equal(plane, ref.to_words(m.vol[k], state)), ("layer", k, state)
        assert np.array_equal(got[3], ref.bool_words(m.changed[k])), ("changed", k)
    assert np.array_equal(c.layer2d(instance), m.layer2d), "layer2d"
    assert np.array_equal(c.origin(instance), m.origin), "origin"


def device_state(c, instance):
    lethal, nonlethal = c.columns(instance)
    return [lethal, nonlethal, c.free_columns(instance), c.layer2d(instance), c.origin(instance)] + list(c.layer_columns(instance, 0)) + list(c.layer_columns(instance, 1))


def same(a, b):
    """lists of device states, instance by instance, array by array"""
    return len(a) == len(b) and all(len(s) == len(t) and all(np.array_equal(x, y) for x, y in zip(s, t)) for s, t in zip(a, b))


def window(m):
    return (m.origin[0], m.origin[1], m.origin[0] + SX * RES, m.origin[1] + SY * RES)


def cycle_after(c, m, instance, seed):
    """what a cycle does behind a roll: the update reports the window once; a new cloud, clipped against the new window; an update"""
    assert tuple(c.update([instance], [ROBOT])[0]) == m.update(ROBOT) == window(m)
    assert_equal_state(c, m, instance)
    rng = np.random.default_rng(seed)
    lo, hi = m.origin - 0.4, m.origin + np.array(SIZE) * RES + 0.4
    pts = np.concatenate([(lo + rng.random((150, 3)) * (hi - lo)), rng.choice(np.array(INTENSITY), (150, 1))], axis=1).astype(np.float32)
    clipped = c.buffer_clouds([(instance, 1, 0, len(pts))], pts)[0]
    assert clipped == m.buffer_cloud(1, pts) and 0 < clipped < len(pts)
    assert_equal_state(c, m, instance)
    assert tuple(c.update([instance], [ROBOT])[0]) == m.update(ROBOT)
    assert_equal_state(c, m, instance)
    bounds = m.update(ROBOT)  # nothing new: the cylinder's columns alone, the mark is long consumed
    assert tuple(c.update([instance], [ROBOT])[0]) == bounds != window(m)
    assert_equal_state(c, m, instance)


SHIFTS = [(1, 0), (-1, 0), (0, 1), (0, -1), (3, -2), (-5, 4), (64, 0), (65, 3), (71, 7), (72, 0), (0, 8), (-100, 50)]


@pytest.mark.parametrize("shift", SHIFTS, ids=[f"{dx},{dy}" for dx, dy in SHIFTS])
def test_one_roll_from_a_fresh_state(nav, prototype, shift):
    c, maps = build(nav, prototype)
    assert_equal_state(c, maps[0])
    others = [device_state(c, i) for i in (1, 2)]
    target = ORIGIN[:2] + np.array(shift) * RES
    got = c.roll([0], origin_xy=[target])
    assert tuple(got[0]) == maps[0].roll_origin(target) == shift
    assert_equal_state(c, maps[0])
    everything_leaves = abs(shift[0]) >= SX or abs(shift[1]) >= SY
    assert bool(maps[0].master.any()) != everything_leaves and bool(maps[0].changed[1].any()) != everything_leaves
    assert same(others, [device_state(c, i) for i in (1, 2)])  # the instances not listed: not a bit moved
    cycle_after(c, maps[0], 0, 7)
    c.close()


def test_a_chain_of_four_rolls_without_an_update(nav, prototype):
    c, maps = build(nav, prototype)
    m, at = maps[2], np.zeros(2, np.int64)
    for step in ((1, 0), (-3, 2), (0, -1), (5, 1)):
        at += step
        target = ORIGIN[:2] + at * RES
        assert tuple(c.roll([2], origin_xy=[target])[0]) == m.roll_origin(target) == step
        assert_equal_state(c, m, 2)
    cycle_after(c, m, 2, 8)
    c.close()


def test_centre_mode_with_the_float_rule_pose(nav, prototype):
    c, maps = build(nav, prototype)
    robots = [(FLOAT_RULE_X, 2.0), (0.3, 1.4), (7.0, 2.0)]  # the third is the window's own centre: (0, 0)
    got = c.roll([0, 1, 2], robot_xy=robots)
    want = [maps[i].roll_centre(robots[i]) for i in range(3)]
    assert [tuple(g) for g in got] == want == [(13, 0), (-27, -3), (0, 0)]
    for i in range(3):
        assert_equal_state(c, maps[i], i)
    assert c.origin(0)[0] == 5 * RES and maps[2].moved is False
    cycle_after(c, maps[1], 1, 9)
    c.close()


def test_a_mixed_list_moves_only_what_moves(nav, prototype):
    c, maps = build(nav, prototype)
    still = [device_state(c, i) for i in (1, 2)]
    targets = [ORIGIN[:2] + np.array([3, -2]) * RES, ORIGIN[:2]]
    got = c.roll([0, 1], origin_xy=targets)
    assert [tuple(g) for g in got] == [maps[0].roll_origin(targets[0]), maps[1].roll_origin(targets[1])] == [(3, -2), (0, 0)]
    assert same(still, [device_state(c, i) for i in (1, 2)])  # shift (0, 0) and not listed: byte for byte as they were
    assert_equal_state(c, maps[0])
    # no moved mark on instance 1: its update reports the pending cloud's bounds, not the window
    bounds = c.update([1, 0], [ROBOT, ROBOT])
    assert tuple(bounds[0]) == maps[1].update(ROBOT) != window(maps[1]) and tuple(bounds[1]) == maps[0].update(ROBOT) == window(maps[0])
    for i in range(3):
        assert_equal_state(c, maps[i], i)
    # reset clears the mark: the full update reports the window either way, and the one after it does not
    target = ORIGIN[:2] + np.array([1, 1]) * RES
    c.roll([2], origin_xy=[target]), maps[2].roll_origin(target)
    c.reset([2]), maps[2].reset()
    assert tuple(c.update([2], [ROBOT])[0]) == maps[2].update(ROBOT) == window(maps[2])
    assert tuple(c.update([2], [ROBOT])[0]) == maps[2].update(ROBOT) != window(maps[2])  # (the cylinder's columns)
    assert_equal_state(c, maps[2], 2)
    c.close()


def test_distance_query_on_the_rolled_master(nav, prototype):
    c, maps = build(nav, prototype)
    m = maps[0]
    c.update([0], [ROBOT]), m.update(ROBOT)
    target = ORIGIN[:2] + np.array([-6, 2]) * RES
    c.roll([0], origin_xy=[target]), m.roll_origin(target)
    cells = np.argwhere(m.master == ref.LETHAL)
    assert 5 < len(cells) < 120
    centres = qref.cell_centres(cells, m.origin, RES)
    assert c.set_mesh(qref.TETRA_VERTICES, qref.TETRA_TRIANGLES) is True
    rng = np.random.default_rng(11)
    poses = [list(rng.uniform(m.origin, m.origin + np.array([SX, SY, 24]) * RES)) + [0.0, 0.0, 0.0, 1.0] for _ in range(10)]
    poses += [list(centres[0]) + [0.0, 0.0, 0.0, 1.0]]
    want = np.array([qref.query_pose(centres, RES, qref.TETRA_VERTICES, qref.TETRA_TRIANGLES, np.asarray(p), mode=qref.DISTANCE) for p in poses])
    got, _ = c.query(poses, mode=qref.DISTANCE)
    assert np.array_equal(got < 0, want < 0) and (want < 0).any() and (want > 0).any()
    assert np.all(np.abs(got[want >= 0] - want[want >= 0]) <= 1e-9) and np.array_equal(got[want < 0], want[want < 0])  # the query's own bound
    f = nav.Costmap3D(1, SX, SY, SZ, RES, max_triangles=16, max_boxes=256, max_poses=64)  # a fresh handle at the new origin
    f.set_origin(0, m.origin)
    f.set_columns(0, ref.to_words(m.master, ref.LETHAL), ref.to_words(m.master, ref.NONLETHAL))
    f.set_mesh(qref.TETRA_VERTICES, qref.TETRA_TRIANGLES)
    assert np.array_equal(f.query(poses, mode=qref.DISTANCE)[0], got)
    f.close()
    c.close()


def test_roll_on_a_handle_without_layers(nav, prototype):
    c = nav.Costmap3D(2, SX, SY, SZ, RES, max_triangles=16, max_boxes=256, max_poses=64)
    planes = [(ref.to_words(m.master, ref.LETHAL), ref.to_words(m.master, ref.NONLETHAL)) for m in prototype[:2]]
    for i in (0, 1):
        c.set_origin(i, ORIGIN)
        c.set_columns(i, *planes[i])
    want, at = list(planes[1]), np.zeros(2, np.int64)
    for shift in ((3, -2), (-67, 1), (0, 0), (0, 9)):  # the last one empties the map
        at += shift
        target = ORIGIN[:2] + at * RES
        assert tuple(c.roll([1], origin_xy=[target])[0]) == shift
        want = [roll.shifted(p.T, shift[0], shift[1], 0).T for p in want]
        assert bool(want[0].any()) == (shift != (0, 9))
        got = c.columns(1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), shift
        assert np.array_equal(c.origin(1), [target[0], target[1], ORIGIN[2]])
        still = c.columns(0)
        assert np.array_equal(still[0], planes[0][0]) and np.array_equal(still[1], planes[0][1]) and np.array_equal(c.origin(0), ORIGIN)
    c.close()


def test_reset_bounding_box(nav, prototype):
    c, maps = build(nav, prototype)
    hi = ORIGIN + np.array(SIZE) * RES
    # crosses the tile boundary at column 64 and is clipped by the window on two sides: columns 40..71 and beyond, rows below 0..4
    # and levels 1..62
    box = (ORIGIN[0] + 40.5 * RES, ORIGIN[1] - 3.0, ORIGIN[2] + 1.01 * RES, hi[0] + 2.0, ORIGIN[1] + 4.99 * RES, hi[2] - RES - 0.01)
    one_cell = tuple(centre_of((64, 7, 0))) * 2                                   # both ends inclusive: one point, one cell
    assert maps[2].vol[1][64, 7, 0] != ref.ABSENT and not maps[2].changed[1][64, 7, 0]
    outside = (hi[0] + 0.01, ORIGIN[1], ORIGIN[2], hi[0] + 5.0, hi[1], hi[2])
    before = maps[0].vol[1].copy()
    # a mixed list, the mask naming the cloud layer and the static layer (which ignores the call)
    c.reset_bounding_box([2, 0, 1], [one_cell, box, outside], [0, 1])
    maps[2].reset_bounding_box(one_cell, [0, 1]), maps[0].reset_bounding_box(box, [0, 1]), maps[1].reset_bounding_box(outside, [0, 1])
    assert (before[40:, 0:5, :] != ref.ABSENT).sum() > (maps[0].vol[1][40:, 0:5, :] != ref.ABSENT).sum() > 0  # levels 0 and 63 stay
    assert maps[2].vol[1][64, 7, 0] == ref.ABSENT and maps[2].changed[1][64, 7, 0]
    for i in range(3):
        assert_equal_state(c, maps[i], i)
    bounds = c.update([0, 1, 2], [ROBOT] * 3)
    for i in range(3):
        assert tuple(bounds[i]) == maps[i].update(ROBOT)
        assert_equal_state(c, maps[i], i)
    # nothing named that holds cells, min > max, and a second time: nothing changes
    state = [device_state(c, i) for i in range(3)]
    c.reset_bounding_box([0], [box], [0, 2])
    c.reset_bounding_box([0], [box[3:] + box[:3]], [1])
    c.reset_bounding_box([0, 2], [box, one_cell], [1])
    assert same(state, [device_state(c, i) for i in range(3)])
    assert tuple(c.update([0], [ROBOT])[0]) == maps[0].update(ROBOT)
    # behind a roll: the box is clipped against the new window
    target = ORIGIN[:2] + np.array([-30, 3]) * RES
    c.roll([0], origin_xy=[target]), maps[0].roll_origin(target)
    low = (ORIGIN[0], ORIGIN[1] + 3 * RES, ORIGIN[2], ORIGIN[0] + 20.5 * RES, ORIGIN[1] + 4.5 * RES, hi[2])  # columns 30..50 of rows 0, 1 now
    c.reset_bounding_box([0], [low], [1]), maps[0].reset_bounding_box(low, [1])
    assert maps[0].changed[1][30:51, 0:2].any() and not maps[0].changed[1][:30].any() and not maps[0].changed[1][:, 2:].any()
    assert_equal_state(c, maps[0])
    cycle_after(c, maps[0], 0, 12)
    c.close()


def test_a_row_wider_than_the_x_pass_holds_at_a_time(nav):
    """k_c3d_roll_x holds 2048 columns of a row in registers; a row one tile wider goes in two chunks, in the direction of dx"""
    limit = 2048
    sx, sy = limit + 64, 2
    rng = np.random.default_rng(13)
    planes = [rng.integers(0, 1 << 63, (sy, sx), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (sy, sx), dtype=np.uint64) for _ in range(2)]
    planes[1] &= ~planes[0]
    c = nav.Costmap3D(1, sx, sy, SZ, RES, max_triangles=16, max_boxes=16, max_poses=16)
    c.set_origin(0, ORIGIN)
    c.configure_layers([dict(max_cloud_points=64, **XYZI)])
    c.set_columns(0, *planes)
    at = 0
    for dx in (1, -(limit + 1)):
        at += dx
        assert tuple(c.roll([0], origin_xy=[ORIGIN[:2] + np.array([at, 0]) * RES])[0]) == (dx, 0)
        planes = [roll.shifted(p.T, dx, 0, 0).T for p in planes]
        got = c.columns(0)
        assert planes[0].any() and np.array_equal(got[0], planes[0]) and np.array_equal(got[1], planes[1]), dx
    assert (c.layer2d(0) == 255).all() and not c.free_columns(0).any()
    c.close()


def test_error_cases_change_nothing_resident(nav, prototype):
    from navigation_amd import NavgpuError
    c, maps = build(nav, prototype)
    before = [device_state(c, i) for i in range(3)]
    hi = ORIGIN + np.array(SIZE) * RES
    box = tuple(ORIGIN) + tuple(hi)
    bad_calls = [
        lambda: c.roll([3], robot_xy=[(0.0, 0.0)]),
        lambda: c.roll([1, 1], robot_xy=[(0.0, 0.0)] * 2),
        lambda: c.roll([0, 1], robot_xy=[(0.0, 0.0), (np.nan, 0.0)]),
        lambda: c.roll([0, 1], origin_xy=[(0.0, 0.0), (0.1, 0.0)]),                      # unaligned
        lambda: c.roll([0, 1], origin_xy=[(0.0, 0.0), (0.25 * 2.0 ** 31, 0.0)]),
        lambda: c.reset_bounding_box([3], [box], [1]),
        lambda: c.reset_bounding_box([0, 0], [box, box], [1]),
        lambda: c.reset_bounding_box([0], [box], [3]),                                   # a layer that is not configured
        lambda: c.reset_bounding_box([0, 1], [box, (np.inf,) + box[1:]], [1]),
    ]
    for call in bad_calls:
        with pytest.raises(NavgpuError):
            call()
    c.set_origin(2, ORIGIN + np.array([0.1, 0.0, 0.0]))  # an unaligned current origin
    for call in (lambda: c.roll([0, 2], robot_xy=[(0.0, 0.0)] * 2), lambda: c.reset_bounding_box([0, 2], [box, box], [1])):
        with pytest.raises(NavgpuError):
            call()
    c.set_origin(2, ORIGIN)
    assert same(before, [device_state(c, i) for i in range(3)])
    for i in range(3):
        assert_equal_state(c, maps[i], i)
    c.close()
