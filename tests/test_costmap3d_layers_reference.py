"""The numpy yardstick of the layered costmap_3d update (tests/costmap3d_layers_ref.py) against closed forms: what the GPU tests compare
the kernels with must itself say what include/navgpu_costmap3d_layers.h says.  Everything is integers, bytes, or doubles from
binary-exact expressions (cells of 0.25 m, origins that are multiples of it), so every comparison is equality.  No GPU."""
import itertools

import numpy as np
import pytest

import costmap3d_layers_ref as ref

RES = 0.25
ORIGIN = np.array([-2.0, 1.0, -0.5])
SIZE = (8, 8, 8)


def cells_of(vol):
    return {tuple(int(v) for v in c): int(vol[tuple(c)]) for c in np.argwhere(vol != ref.ABSENT)}


def test_a_point_on_a_cell_face_goes_to_the_upper_cell():
    ok = ref.origin_keys(ORIGIN, RES)
    assert list(ok) == [-8, 4, -2]
    # x = -1.5 is the face between cells 1 and 2; just below it is cell 1
    vol, clipped = ref.cloud_cells([[-1.5, 1.0, -0.5], [np.nextafter(np.float32(-1.5), np.float32(-2.0)), 1.0, -0.5]], SIZE, ORIGIN, RES)
    assert cells_of(vol) == {(2, 0, 0): ref.LETHAL, (1, 0, 0): ref.LETHAL} and clipped == 0
    # the upper face of the extents is outside, the lower inside; NaN and inf are dropped
    vol, clipped = ref.cloud_cells([[0.0, 1.0, -0.5], [-2.0, 3.0, -0.5], [-2.0, 1.0, 1.5], [-2.0, 1.0, -0.5], [np.nan, 1.0, 0.0], [0.0, np.inf, 0.0]], SIZE, ORIGIN, RES)
    assert cells_of(vol) == {(0, 0, 0): ref.LETHAL} and clipped == 5
    assert ref.cell_centre(3, ok[0], RES) == -2.0 + 3.5 * RES


def test_transform_is_fp64_stored_as_float():
    c, s = np.cos(0.5), np.sin(0.5)
    tf = (c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0, 0.125, -0.25, 0.5)
    p = np.array([[1.0, 2.0, 3.0]], np.float32)
    got = ref.transform_points(p, tf)
    assert got.dtype == np.float32
    assert got[0, 0] == np.float32(c * 1.0 + -s * 2.0 + 0.0 * 3.0 + 0.125) and got[0, 2] == np.float32(3.5)


def test_intensity_classes():
    free, lethal = 0.25, 0.75
    cls = lambda i: ref.cost_class(ref.intensity_cost(i, free, lethal))
    assert cls(0.75) == ref.LETHAL and cls(2.0) == ref.LETHAL
    assert cls(0.25) == ref.FREE and cls(-1.0) == ref.FREE
    assert cls(0.5) == ref.NONLETHAL and ref.intensity_cost(0.5, free, lethal) == np.float32(0.0)
    # a value strictly below the lethal intensity whose float Cost rounds to 10: with free = -1000 the subtraction i - free rounds to
    # lethal - free, the ratio is 1 and the Cost 10 - LETHAL by the Cost, although the first test (i >= lethal) did not hold
    just_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert just_below < np.float32(1.0)
    cost = ref.intensity_cost(just_below, -1000.0, 1.0)
    assert cost.dtype == np.float32 and cost == np.float32(10.0) and ref.cost_class(cost) == ref.LETHAL
    assert ref.intensity_cost(np.nextafter(np.float32(0.75), np.float32(0.0)), free, lethal) == np.float32(9.999998)
    # and one that does not
    assert cls(np.float32(0.74)) == ref.NONLETHAL
    just_above = np.nextafter(np.float32(0.25), np.float32(1.0))
    assert ref.intensity_cost(just_above, free, lethal) > np.float32(-10.0) and cls(just_above) == ref.NONLETHAL


def test_highest_class_per_cell():
    pts = [[-1.9, 1.1, -0.4, 0.5], [-1.9, 1.1, -0.4, 1.0], [-1.9, 1.1, -0.4, 0.0], [-1.6, 1.1, -0.4, 0.0], [-1.6, 1.1, -0.4, 0.5], [-1.4, 1.1, -0.4, 0.0]]
    for order in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [1, 0, 2, 4, 3, 5]):
        vol, _ = ref.cloud_cells([pts[k] for k in order], SIZE, ORIGIN, RES, has_intensity=True, free_intensity=0.25, lethal_intensity=0.75)
        assert cells_of(vol) == {(0, 0, 0): ref.LETHAL, (1, 0, 0): ref.NONLETHAL, (2, 0, 0): ref.FREE}


def test_replace_semantics():
    m = ref.LayeredMap(SIZE, ORIGIN, RES, [dict(kind=ref.POINT_CLOUD, cloud_has_intensity=1, free_intensity=0.25, lethal_intensity=0.75)])
    m.buffer_cloud(0, [[-1.9, 1.1, -0.4, 1.0], [-1.6, 1.1, -0.4, 1.0], [-1.4, 1.1, -0.4, 0.5]])
    assert cells_of(m.changed[0].astype(np.uint8)) == {(0, 0, 0): 1, (1, 0, 0): 1, (2, 0, 0): 1}
    m.changed[0][:] = False
    # cell 0 is not in the second cloud: gone and changed; cell 1 is unchanged: not marked; cell 2 changes class; cell 3 is new
    m.buffer_cloud(0, [[-1.6, 1.1, -0.4, 1.0], [-1.4, 1.1, -0.4, 1.0], [-1.1, 1.1, -0.4, 0.0]])
    assert cells_of(m.vol[0]) == {(1, 0, 0): ref.LETHAL, (2, 0, 0): ref.LETHAL, (3, 0, 0): ref.FREE}
    assert cells_of(m.changed[0].astype(np.uint8)) == {(0, 0, 0): 1, (2, 0, 0): 1, (3, 0, 0): 1}


@pytest.mark.parametrize("method", [ref.OVERWRITE, ref.MAXIMUM, ref.IF_UNKNOWN, ref.NOTHING])
def test_combination_methods_over_all_state_pairs(method):
    """a 2-layer stack: the lower layer (Overwrite) puts state a into cell (a, b, 0), the upper one state b with the method under test"""
    states = [ref.ABSENT, ref.FREE, ref.NONLETHAL, ref.LETHAL]
    m = ref.LayeredMap(SIZE, ORIGIN, RES, [dict(kind=ref.POINT_CLOUD, combination_method=ref.OVERWRITE), dict(kind=ref.POINT_CLOUD, combination_method=method)])
    for a, b in itertools.product(states, states):
        m.vol[0][a, b, 0], m.vol[1][a, b, 0] = a, b
    m.update((0.0, 0.0, 0.0))  # the first update after configure: everything is bounds
    for a, b in itertools.product(states, states):
        want = {ref.OVERWRITE: b if b != ref.ABSENT else a, ref.MAXIMUM: max(a, b), ref.IF_UNKNOWN: a if a != ref.ABSENT else b, ref.NOTHING: a}[method]
        assert m.master[a, b, 0] == want, (method, a, b)


def test_cylinder_erases_and_its_previous_set_is_restored():
    layers = [dict(kind=ref.STATIC_2D, height=-0.5, lethal_cost_threshold=100), dict(kind=ref.CYLINDER_CLEARING, radius=0.3)]
    m = ref.LayeredMap(SIZE, ORIGIN, RES, layers)
    m.set_static_grid(0, np.full((8, 8), 100, np.int8), -2.0, 1.0)
    # round (-1.125, 1.875) - the centre of column (3, 3) - with r = 0.3: the column itself and its 4 neighbours (0.25 away; the diagonal is 0.354)
    cols = ref.cylinder_columns((-1.125, 1.875), 0.3, SIZE, ORIGIN, RES)
    assert {tuple(c) for c in np.argwhere(cols)} == {(3, 3), (2, 3), (4, 3), (3, 2), (3, 4)}
    m.update((-1.125, 1.875, 0.0))
    assert (m.master[:, :, 0] == ref.LETHAL).sum() == 64 - 5 and np.all(m.master[cols] == ref.ABSENT)
    assert m.layer2d[3, 3] == 255 and m.layer2d[0, 0] == 254
    # the robot moves two columns on: the old set comes back from the static layer, the new one is erased; nothing else is in bounds
    m.master[7, 7, 5] = ref.NONLETHAL  # a sentinel outside bounds
    b = m.update((-0.625, 1.875, 0.0))
    now = ref.cylinder_columns((-0.625, 1.875), 0.3, SIZE, ORIGIN, RES)
    assert np.all(m.master[:, :, 0][~now] == ref.LETHAL) and np.all(m.master[now] == ref.ABSENT) and m.master[7, 7, 5] == ref.NONLETHAL
    assert b == (-2.0 + 2 * RES, 1.0 + 2 * RES, -2.0 + 7 * RES, 1.0 + 5 * RES)
    # disabled: the previous set is added once more and then forgotten
    m.layer_set(1, 0, ref.MAXIMUM)
    assert m.update((0.0, 0.0, 0.0)) == (-2.0 + 4 * RES, 1.0 + 2 * RES, -2.0 + 7 * RES, 1.0 + 5 * RES)
    assert (m.master[:, :, 0] == ref.LETHAL).all()
    assert m.update((0.0, 0.0, 0.0)) == ref.EMPTY_BOUNDS


def test_projection_bytes_and_bounds():
    col = np.zeros(8, np.uint8)
    assert ref.project_column(col) == 255
    col[3] = ref.FREE
    assert ref.project_column(col) == 0
    col[5] = ref.NONLETHAL
    assert ref.project_column(col) == 127 and ref.project_column(col, 99) == 99
    col[0] = ref.LETHAL
    assert ref.project_column(col) == 254
    m = ref.LayeredMap(SIZE, ORIGIN, RES, [dict(kind=ref.POINT_CLOUD, cloud_has_intensity=1, free_intensity=0.25, lethal_intensity=0.75)])
    assert m.update((0.0, 0.0, 0.0)) == (-2.0, 1.0, 0.0, 3.0) and np.all(m.layer2d == 255)  # full: the whole map
    assert m.update((0.0, 0.0, 0.0)) == ref.EMPTY_BOUNDS == (1e6, 1e6, -1e6, -1e6)
    m.buffer_cloud(0, [[-1.6, 1.3, 0.0, 1.0], [-0.9, 2.6, 0.3, 0.5], [-0.9, 2.6, 1.0, 0.0]])
    assert m.update((0.0, 0.0, 0.0)) == (-2.0 + 1 * RES, 1.0 + 1 * RES, -2.0 + 5 * RES, 1.0 + 7 * RES)
    assert m.layer2d[1, 1] == 254 and m.layer2d[6, 4] == 127 and (m.layer2d != 255).sum() == 2
    m.buffer_cloud(0, [[-0.9, 2.6, 1.0, 0.0]])
    assert m.update((0.0, 0.0, 0.0)) == (-2.0 + 1 * RES, 1.0 + 1 * RES, -2.0 + 5 * RES, 1.0 + 7 * RES)
    assert m.layer2d[1, 1] == 255 and m.layer2d[6, 4] == 0


def test_update_costs_over_all_byte_pairs():
    for master, layer in itertools.product(range(256), range(256)):
        # updateWithMax: NO_INFORMATION in the layer never writes; in the master it always yields; else the larger
        want_max = master if layer == 255 else layer if master == 255 else max(master, layer)
        want_over = master if layer == 255 else layer
        assert ref.update_with_max(master, layer) == want_max and ref.update_with_overwrite(master, layer) == want_over
    master = np.arange(64, dtype=np.uint8).reshape(8, 8)
    layer = np.full((8, 8), 200, np.uint8)
    layer[2, 2] = 255
    for use_max, inside in ((True, 200), (False, 200)):
        out = ref.update_costs(master, layer, (1, 2, 4, 5), use_max)
        assert out[2, 1] == inside and out[2, 2] == master[2, 2] and out[1, 1] == master[1, 1] and out[5, 1] == master[5, 1] and out[2, 4] == master[2, 4]


def test_static_grid_values():
    grid = np.array([[-1, 0], [99, 100]], np.int8)
    for utl, want in ((False, {(1, 0, 2): ref.FREE, (0, 1, 2): ref.FREE, (1, 1, 2): ref.LETHAL}),
                      (True, {(0, 0, 2): ref.LETHAL, (1, 0, 2): ref.FREE, (0, 1, 2): ref.FREE, (1, 1, 2): ref.LETHAL})):
        vol, clipped = ref.static_cells(grid, -2.0, 1.0, SIZE, ORIGIN, RES, 0.1, 100, utl)
        assert cells_of(vol) == want and clipped == 0
    vol, clipped = ref.static_cells(grid, -2.25, 1.0, SIZE, ORIGIN, RES, 0.1, 100, True)  # the first column lies off the extents
    assert cells_of(vol) == {(0, 0, 2): ref.FREE, (0, 1, 2): ref.LETHAL} and clipped == 2
    vol, clipped = ref.static_cells(grid, -2.0, 1.0, SIZE, ORIGIN, RES, 1.5, 100, False)  # the level is: every cell that would be made
    assert not vol.any() and clipped == 3


def test_words_are_bit_planes():
    vol = np.zeros((3, 2, 64), np.uint8)
    vol[2, 1, 63], vol[0, 0, 0], vol[1, 0, 5] = ref.LETHAL, ref.LETHAL, ref.FREE
    w = ref.to_words(vol, ref.LETHAL)
    assert w.shape == (2, 3) and w[1, 2] == np.uint64(1) << np.uint64(63) and w[0, 0] == 1 and w.sum() == w[1, 2] + np.uint64(1)
    assert ref.to_words(vol, ref.FREE)[0, 1] == 32
