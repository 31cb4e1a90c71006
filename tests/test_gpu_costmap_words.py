"""k_merge's word-parallel instantiations and k_inflate_bits' mask-style phases at the places their new paths can go wrong (need a real
MI355X): update boxes at every column residue and width of a 16-cell group on a map whose rows hold whole groups (48 wide) and on one whose
groups straddle rows (50 wide); seeds at tile corners, on the grown box's edges, one cell outside it, in the first and last halo row only,
a tile full of seeds and a box without any, for inflation radii 1, 5, 11 (the compiled radius) and 14 cells with more than eight robots in
a launch.  Expected bytes: tests/byte_rules_ref.py for the merges, oracle.pyoracle.inflate(exact=True) for the inflation.  Everything is
bytes: every comparison is np.array_equal."""
import numpy as np
import pytest

import byte_rules_ref as R
from test_gpu_parity import L, nav  # noqa: F401

pytestmark = pytest.mark.gpu

SPECIAL = np.array([0, 1, 127, 252, 253, 254, 255], np.uint8)
WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 33)
MERGE_GEOMETRIES = [(40, 48), (40, 50)]  # ny, nx: rows of whole 16-cell groups; groups that straddle rows


def _layer_bytes(rs, shape):
    """half the cells from the values the rules single out, half uniform"""
    out = rs.randint(0, 256, shape).astype(np.uint8)
    pick = rs.rand(*shape) < 0.5
    out[pick] = SPECIAL[rs.randint(0, len(SPECIAL), int(pick.sum()))]
    return out


def _merge_boxes(ny, nx):
    """x0, y0, xn, yn: every first column 0..17 with every width, boxes that touch each edge of the map, one cell in each corner"""
    boxes = []
    for x0 in range(18):
        for w in WIDTHS:
            y0 = (3 * x0 + w) % 7
            boxes.append((x0, y0, min(x0 + w, nx), min(y0 + 1 + (5 * x0 + w) % 31, ny)))
    boxes += [(0, 0, nx, 1), (0, ny - 1, nx, ny), (0, 0, 1, ny), (nx - 1, 0, nx, ny), (nx - 17, 3, nx, ny), (0, 0, nx, ny),
              (0, 0, 1, 1), (nx - 1, ny - 1, nx, ny), (15, 0, 17, ny), (16, 1, 32, ny - 1), (31, 2, 33, 3)]
    return boxes


def _world(boxes):
    """the boxes as CostmapLayer::resetBoundingBox takes them at 1 m / cell (the maximum is inclusive)"""
    return np.array([(x0 + 0.5, y0 + 0.5, xn - 0.5, yn - 0.5) for x0, y0, xn, yn in boxes])


@pytest.mark.parametrize("ny,nx", MERGE_GEOMETRIES)
@pytest.mark.parametrize("track_unknown", [False, True])
@pytest.mark.parametrize("with_static", [False, True])
def test_merge_boxes_every_residue(nav, ny, nx, track_unknown, with_static):
    """reset -> static rule -> obstacle rule over one box per robot (the last robot has none: its box is empty), for use_maximum x
    combination_method 0 / 1 / 2 (2: the obstacle layer merges nothing), with and without a static layer; outside the box the
    sentinel master stays."""
    N = L(nav)
    boxes = _merge_boxes(ny, nx)
    nb, n = len(boxes), len(boxes) + 1
    rs = np.random.RandomState(1000 * nx + 10 * int(track_unknown) + int(with_static))
    layers = N.LAYER_OBSTACLE | (N.LAYER_STATIC if with_static else 0)
    fl = nav.Fleet(n, nx, ny, 1.0, layers=layers, track_unknown=track_unknown, max_points=16, max_observations=1)
    poses = [[0.0, 0.0, 0.0]] * n
    for use_maximum in ((False, True) if with_static else (False,)):
        for comb in (0, 1, 2):
            statics, obst, sentinel = _layer_bytes(rs, (n, ny, nx)), _layer_bytes(rs, (n, ny, nx)), _layer_bytes(rs, (n, ny, nx))
            fl.configure_obstacle(footprint_clearing_enabled=False, combination_method=comb)
            if with_static:  # the layer's first cycle covers the whole map (new data): the box touches every edge
                fl.add_static_map(np.zeros((ny, nx), np.int8), use_maximum=use_maximum)
                fl.upload(N.GRID_STATIC, statics)
                fl.upload(N.GRID_OBSTACLE, obst)
                fl.upload(N.GRID_MASTER, sentinel)
                fl.stage_observations(poses, [])
                fl.update_map()
                got = fl.master()
                for k in (0, 7, n - 1):
                    want = R.update_map(sentinel[k], track_unknown, statics[k], use_maximum, obst[k], comb)
                    assert np.array_equal(got[k], want), ("whole map", use_maximum, comb, k)
            fl.reset_bounding_box(_world(boxes), first=0, count=nb)
            fl.upload(N.GRID_OBSTACLE, obst)  # (resetBoundingBox has reset the layer inside the box)
            fl.upload(N.GRID_MASTER, sentinel)
            fl.stage_observations(poses, [])
            fl.update_map()
            got, bounds = fl.master(), fl.bounds()
            for k, (x0, y0, xn, yn) in enumerate(boxes):
                assert list(bounds[k]) == [x0, xn, y0, yn], (k, boxes[k])
                want = R.update_map(sentinel[k], track_unknown, statics[k] if with_static else None, use_maximum, obst[k], comb, box=boxes[k])
                outside = np.ones((ny, nx), bool)
                outside[y0:yn, x0:xn] = False
                assert np.array_equal(got[k][outside], sentinel[k][outside]), ("outside the box", use_maximum, comb, boxes[k])
                assert np.array_equal(got[k], want), ("box", use_maximum, comb, boxes[k], int((got[k] != want).sum()))
            assert np.array_equal(got[n - 1], sentinel[n - 1]), ("a robot without bounds", use_maximum, comb, list(bounds[n - 1]))
    fl.close()


@pytest.mark.parametrize("ny,nx", MERGE_GEOMETRIES)
@pytest.mark.parametrize("combination_method", [0, 1, 2])
def test_merge_layer_only_boxes_every_residue(nav, ny, nx, combination_method):
    """ObstacleLayer::updateCosts alone (navgpu_obstacle_update_costs) over the same boxes, and over an empty and an inverted one"""
    N = L(nav)
    boxes = _merge_boxes(ny, nx) + [(5, 5, 5, 5), (9, 9, 3, 3), (0, 7, nx, 7)]
    n = len(boxes)
    rs = np.random.RandomState(77 * nx + combination_method)
    masters, obst = _layer_bytes(rs, (n, ny, nx)), _layer_bytes(rs, (n, ny, nx))
    fl = nav.Fleet(n, nx, ny, 1.0, layers=N.LAYER_OBSTACLE, track_unknown=True, max_points=16, max_observations=1)
    fl.configure_obstacle(footprint_clearing_enabled=False, combination_method=combination_method)
    fl.upload(N.GRID_MASTER, masters)
    fl.upload(N.GRID_OBSTACLE, obst)
    fl.obstacle_update_costs(boxes)
    got = fl.master()
    for k in range(n):
        want = R.obstacle_update_costs(masters[k], obst[k], combination_method, boxes[k])
        assert np.array_equal(got[k], want), (boxes[k], int((got[k] != want).sum()))
    assert np.array_equal(fl.download(N.GRID_OBSTACLE), obst)
    fl.close()


# ----------------------------------------------------------------------------------------------
# inflation: k_inflate_bits<11> and the generic radius, 64 x 32 tiles on maps that are no multiple of the tile
# ----------------------------------------------------------------------------------------------
SCALING, INSCRIBED = 0.1, 1.5  # at 1 m / cell: cost 253 up to 1.5 cells, then 251 .. 72 out to 14 cells
BACKGROUND = np.array([0, 0, 0, 1, 50, 100, 200, 252, 253, 255, 255], np.uint8)  # old bytes: NO_INFORMATION, and values above any new cost


def _inflation_cases(ny, nx, Rc, rs):
    """(map, box) per robot; 254 only where a case puts a seed"""
    def ground():
        return BACKGROUND[rs.randint(0, len(BACKGROUND), (ny, nx))]

    def seeds(m, cells):
        for x, y in cells:
            if 0 <= x < nx and 0 <= y < ny:
                m[y, x] = 254
        return m

    whole = (0, 0, nx, ny)
    cases = []
    cases.append((seeds(ground(), [(63, 31), (64, 32)]), whole))                                    # either side of a tile corner
    cases.append((seeds(ground(), [(0, 0), (63, 0), (64, 31), (63, 32), (nx - 1, ny - 1), (0, ny - 1), (nx - 1, 0), (64, 63), (127, 32)]), whole))
    # seeds on the grown box's first and last column and row, and one cell outside each (those must not seed)
    x0, y0, xn, yn = Rc + 20, Rc + 8, nx - Rc - 20, ny - Rc - 8
    edge = [(x0 - Rc, y0 + 3), (xn + Rc - 1, y0 + 9), (x0 + 5, y0 - Rc), (x0 + 11, yn + Rc - 1)]
    outside = [(x0 - Rc - 1, yn - 2), (xn + Rc, yn - 5), (xn - 3, y0 - Rc - 1), (xn - 9, yn + Rc)]
    cases.append((seeds(ground(), edge + outside), (x0, y0, xn, yn)))
    cases.append((seeds(ground(), [(64 + Rc - 1, 10), (20, 32 + Rc - 1), (64 + Rc, 20), (40, 32 + Rc)]), whole))  # within R of tile (0, 0), and one past it
    cases.append((seeds(ground(), [(10, 32 - Rc), (40, 63 + Rc), (70, 32 - Rc)]), whole))           # halo rows 0 and 2R + 31 of tiles (0, 1), (1, 1) only
    full = ground()
    full[32:64, 64:128] = 254                                                                        # a tile full of seeds
    cases.append((full, whole))
    cases.append((ground(), (3, 2, nx - 4, ny - 1)))                                                 # a box without any seed
    sparse = ground()
    sparse[rs.rand(ny, nx) < 0.02] = 254
    cases.append((sparse, (7, 5, nx - 11, ny - 3)))
    dense = ground()
    dense[rs.rand(ny, nx) < 0.3] = 254
    cases.append((dense, whole))
    lines = ground()
    lines[::13, :] = 254                                                                             # seeded rows with seedless rows between
    lines[:, 5] = 254
    cases.append((lines, (0, 0, nx, ny - 9)))
    return cases


@pytest.mark.parametrize("ny,nx", [(80, 96), (70, 130)])
@pytest.mark.parametrize("Rc", [1, 5, 11, 14])
def test_inflate_tiles_boxes_and_seeds(nav, orc, ny, nx, Rc):
    N = L(nav)
    rs = np.random.RandomState(100 * Rc + nx)
    cases = _inflation_cases(ny, nx, Rc, rs)
    n = len(cases)
    assert n >= 9  # robot = 8 z + x % 8 of the launch grid: both sides of it
    maps, boxes = np.stack([m for m, _ in cases]), [b for _, b in cases]
    fl = nav.Fleet(n, nx, ny, 1.0, layers=N.LAYER_INFLATION)
    fl.configure_inflation(float(Rc), SCALING, INSCRIBED)
    fl.upload(N.GRID_MASTER, maps)
    fl.inflate(boxes=boxes)
    got = fl.master()
    fl.close()
    changed = 0
    for k in range(n):
        want = orc.inflate(maps[k], 1.0, float(Rc), SCALING, INSCRIBED, box=boxes[k], exact=True)
        assert np.array_equal(got[k], want), (k, boxes[k], int((got[k] != want).sum()), np.argwhere(got[k] != want)[:4].tolist())
        changed += int((want != maps[k]).sum())
        if k == 6:
            assert np.array_equal(want, maps[k]), "the seedless box changed the map"
    assert changed > 1000
    # the rule of inflation_layer.cpp:243-247 went both ways: NO_INFORMATION gave way to cost >= 253 and stayed below it; old values above the cost stayed
    m, w = maps[8], orc.inflate(maps[8], 1.0, float(Rc), SCALING, INSCRIBED, box=boxes[8], exact=True)
    assert ((m == 255) & (w == 253)).any() and ((m == 255) & (w == 255)).any() and ((m == 253) & (w == 253)).any()
