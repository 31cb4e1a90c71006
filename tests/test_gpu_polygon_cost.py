"""navgpu_costmap_set_polygon_cost and navgpu_move_base_clear_costmap_windows on the GPU against the CPU oracle's
Costmap2D::setConvexPolygonCost (orc_polygon_fill): whole grids are compared for equality, a robot per polygon case in one call.

Two fleets: 64 x 64, and 1100 x 40 whose widest cases span more than the 1024 columns k_set_polygon_cost holds in LDS at a time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NAVGPU_ERR_INVALID, NAVGPU_ERR_CAPACITY = -1, -4
RES = 0.05
SIZES = [(64, 64), (1100, 40)]


def _ngon(cx, cy, rx, ry, n, phase=0.1):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1)


def _star(cx, cy, rx, ry):
    a = 0.2 + 2 * np.pi * np.arange(10) / 10
    r = np.where(np.arange(10) % 2 == 0, 1.0, 0.4)
    return np.stack([cx + r * rx * np.cos(a), cy + r * ry * np.sin(a)], 1)


def _window(x, y, size_x, size_y):
    """MoveBase::clearCostmapWindows' polygon (move_base.cpp:288-302), in its expressions"""
    return np.array([[x - size_x / 2, y - size_y / 2], [x + size_x / 2, y - size_y / 2], [x + size_x / 2, y + size_y / 2],
                     [x - size_x / 2, y + size_y / 2]])


def _slow_and_clear(x, y, d):
    """MoveSlowAndClear::runBehavior's polygon (move_slow_and_clear.cpp:89-97)"""
    pts = []
    for i in (-1, 1):
        pts.append([x + i * d, y + i * d])
        pts.append([x + i * d, y + -1.0 * i * d])
    return np.array(pts)


def _cases(nx, ny):
    """(name, polygon (k, 2) in the world); the map's origin is (0, 0)"""
    w, h = nx * RES, ny * RES
    cx, cy = w / 2, h / 2
    rs = np.random.RandomState(5 + nx)
    c = []
    for t in range(3):
        c.append((f"triangle {t}", rs.uniform([0, 0], [w, h], (3, 2))))
    c.append(("clearCostmapWindows rectangle", _window(cx + 0.013, cy - 0.021, 1.0, 0.6)))
    c.append(("empty polygon between two robots with polygons", np.zeros((0, 2))))
    c.append(("MoveSlowAndClear polygon", _slow_and_clear(cx - 0.2, cy + 0.07, 0.5)))
    c.append(("64-gon", _ngon(cx, cy, 0.45 * min(w, h), 0.45 * min(w, h), 64)))
    c.append(("256-gon: NAVGPU_MAX_POLYGON", _ngon(cx, cy, 0.49 * w, 0.49 * h, 256)))
    c.append(("non-convex: an arrow head", np.array([[0.1 * w, 0.1 * h], [0.9 * w, 0.5 * h], [0.1 * w, 0.9 * h], [0.6 * w, 0.5 * h]])))
    c.append(("non-convex: a star", _star(cx, cy, 0.4 * w, 0.4 * h)))
    c.append(("all vertices in one cell", np.array([[1.001, 0.501], [1.04, 0.51], [1.02, 0.549], [1.03, 0.52]])))
    c.append(("2 vertices", np.array([[0.3, 0.3], [1.2, 0.9]])))
    c.append(("1 vertex", np.array([[0.3, 0.3]])))
    c.append(("one vertex off the map", np.array([[0.5, 0.5], [-0.01, 0.7], [1.5, 1.5]])))
    c.append(("one vertex beyond the far edge", np.array([[0.5, 0.5], [w, 0.7], [1.5, 1.5]])))
    c.append(("2 vertices, one off the map", np.array([[0.5, 0.5], [0.5, h + 1.0]])))
    c.append(("a NaN vertex", np.array([[0.5, 0.5], [np.nan, 0.7], [1.5, 1.5]])))
    c.append(("the whole map", np.array([[0.0, 0.0], [w - 1e-9, 0.0], [w - 1e-9, h - 1e-9], [0.0, h - 1e-9]])))
    c.append(("a sliver across every column", np.array([[0.01, 0.3], [w - 0.01, h - 0.3], [w - 0.01, h - 0.26]])))
    c.append(("a vertical line of three vertices", np.array([[0.52, 0.1], [0.52, h - 0.1], [0.52, 0.9]])))
    c.append(("wide ellipse", _ngon(cx, cy, 0.48 * w, 0.3 * h, 64)))
    return c


@pytest.fixture(scope="module", params=SIZES, ids=[f"{a}x{b}" for a, b in SIZES])
def setup(request, orc):
    """the cases, the grids every robot starts from, and the oracle's grids and return values per written value: computed once"""
    nx, ny = request.param
    cases = _cases(nx, ny)
    if nx > 1024:
        assert any(np.ptp(np.floor(p[:, 0] / RES)) >= 1024 for _, p in cases if len(p) >= 3), "no case spans more than 1024 columns"
    start = np.random.RandomState(3).randint(0, 256, (len(cases), ny, nx)).astype(np.uint8)
    want = {}
    for value in (0, 254, 255):
        grids, oks = start.copy(), []
        for k, (_, poly) in enumerate(cases):
            g = np.ascontiguousarray(grids[k])
            oks.append(bool(orc.lib().orc_polygon_fill(g, nx, ny, RES, 0.0, 0.0, np.ascontiguousarray(poly, np.float64), len(poly), value)))
            grids[k] = g
        grids.setflags(write=False)
        want[value] = (grids, oks)
    start.setflags(write=False)
    names = [n for n, _ in cases]
    assert [want[0][1][names.index(n)] for n in ("2 vertices", "1 vertex", "empty polygon between two robots with polygons")] == [True] * 3
    assert not any(want[0][1][names.index(n)] for n in ("one vertex off the map", "one vertex beyond the far edge", "2 vertices, one off the map",
                                                       "a NaN vertex"))
    return nx, ny, cases, start, want


def _fleet(nx, ny, n):
    import navigation_amd as nav
    from navigation_amd import _lib as N
    return nav.Fleet(n, nx, ny, RES, layers=N.LAYER_OBSTACLE)


@pytest.mark.parametrize("value", [0, 254, 255])
def test_polygon_cost_matches_the_oracle_on_whole_grids(setup, value):
    from navigation_amd import _lib as N
    nx, ny, cases, start, want = setup
    fl = _fleet(nx, ny, len(cases))
    try:
        for grid, other in ((N.GRID_MASTER, N.GRID_OBSTACLE), (N.GRID_OBSTACLE, N.GRID_MASTER)):
            fl.upload(N.GRID_MASTER, start)
            fl.upload(N.GRID_OBSTACLE, start)
            ok = fl.set_polygon_cost(grid, [p for _, p in cases], value)
            got = fl.download(grid)
            grids, oks = want[value]
            for k, (name, poly) in enumerate(cases):
                assert ok[k] == oks[k], (name, ok[k])
                assert np.array_equal(got[k], grids[k]), (name, int(np.count_nonzero(got[k] != grids[k])))
                if not oks[k] or len(poly) < 3:
                    assert np.array_equal(got[k], start[k]), name
            assert np.array_equal(fl.download(other), start), "the other grid was written"
    finally:
        fl.close()


def test_sub_range_and_limits(setup):
    """a range inside the fleet writes only its robots; more than NAVGPU_MAX_POLYGON vertices and a bad grid are refused, nothing written"""
    import ctypes as C
    from navigation_amd import _lib as N
    nx, ny, cases, start, want = setup
    fl = _fleet(nx, ny, len(cases))
    try:
        fl.upload(N.GRID_MASTER, start)
        fl.upload(N.GRID_OBSTACLE, start)
        ok = fl.set_polygon_cost(N.GRID_MASTER, [p for _, p in cases[2:7]], 254, first=2)
        got = fl.master()
        grids, oks = want[254]
        assert ok == oks[2:7]
        for k in range(len(cases)):
            assert np.array_equal(got[k], grids[k] if 2 <= k < 7 else start[k]), k
        fl.upload(N.GRID_MASTER, start)
        big = np.ascontiguousarray(_ngon(1.0, 1.0, 0.5, 0.5, N.MAX_POLYGON + 1))
        off = np.array([0, 3, 3 + len(big)], np.uint32)
        xy = np.ascontiguousarray(np.concatenate([cases[0][1], big]))
        okv = (C.c_int32 * 2)(7, 7)
        L = fl.L
        assert L.navgpu_costmap_set_polygon_cost(fl.h, N.GRID_MASTER, 0, 2, xy.ctypes.data, off.ctypes.data, 0, okv) == NAVGPU_ERR_CAPACITY
        assert L.navgpu_costmap_set_polygon_cost(fl.h, N.GRID_STATIC, 0, 1, xy.ctypes.data, off.ctypes.data, 0, okv) == NAVGPU_ERR_INVALID
        assert L.navgpu_costmap_set_polygon_cost(fl.h, N.GRID_PATH, 0, 1, xy.ctypes.data, off.ctypes.data, 0, okv) == NAVGPU_ERR_INVALID
        bad = np.array([3, 0], np.uint32)
        assert L.navgpu_costmap_set_polygon_cost(fl.h, N.GRID_MASTER, 0, 1, xy.ctypes.data, bad.ctypes.data, 0, okv) == NAVGPU_ERR_INVALID
        assert list(okv) == [7, 7] and np.array_equal(fl.master(), start)
    finally:
        fl.close()


def test_clear_costmap_windows(setup, orc):
    from navigation_amd import _lib as N
    nx, ny, cases, start, _ = setup
    w, h = nx * RES, ny * RES
    poses = np.array([[w / 2, h / 2], [0.7, 0.8], [w - 0.6, h - 0.7], [0.3, 0.3]])  # the last: the window leaves the map, nothing is cleared
    fl = _fleet(nx, ny, len(poses))
    try:
        fl.upload(N.GRID_MASTER, start[:len(poses)])
        fl.upload(N.GRID_OBSTACLE, start[:len(poses)])
        ok = fl.clear_costmap_windows(poses, 1.1, 0.9)
        got = fl.master()
        for k, (x, y) in enumerate(poses):
            g = start[k].copy()
            want_ok = bool(orc.lib().orc_polygon_fill(g, nx, ny, RES, 0.0, 0.0, np.ascontiguousarray(_window(x, y, 1.1, 0.9)), 4, 0))
            assert ok[k] == want_ok == (k < 3) and np.array_equal(got[k], g), k
            assert np.count_nonzero(got[k] != start[k]) > 0 or k == 3
        assert np.array_equal(fl.download(N.GRID_OBSTACLE), start[:len(poses)])
    finally:
        fl.close()


def test_costmap_update_around_a_polygon_write_is_unchanged(orc):
    """k_obstacle with footprint clearing before and after the new call: a twin fleet that never makes it, and gets the same bytes through
    a download, the oracle's fill and an upload, stays equal to the fleet that does - grids and bounds."""
    import navigation_amd as nav
    from navigation_amd import _lib as N, synth
    n, nI = 64, 2
    insc = synth.inscribed_radius(synth.FOOTPRINT)
    fleets = []
    for _ in range(2):
        fl = nav.Fleet(nI, n, n, RES, layers=N.LAYER_OBSTACLE | N.LAYER_INFLATION, max_points=720)
        fl.configure_obstacle(footprint_clearing_enabled=True)
        fl.set_footprint(synth.FOOTPRINT)
        fl.configure_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, insc)
        fleets.append(fl)
    a, twin = fleets
    insts = [synth.make_instance(n, 70 + i, density=0.02) for i in range(nI)]
    poly = [_slow_and_clear(1.6 + 0.2 * i, 1.5, 0.5) for i in range(nI)]
    try:
        for cyc in range(3):
            poses, obs = [], []
            for i, ins in enumerate(insts):
                pts = synth.laser_scan(ins, cyc, n_beams=180, max_range=3.0)
                org = (float(ins["pos"][0]), float(ins["pos"][1]), 0.3)
                obs.append(dict(instance=i, points=pts, origin=org, obstacle_range=2.5, raytrace_range=3.0))
                poses.append([float(v) + 0.05 * cyc for v in ins["pos"]])
            for fl in fleets:
                fl.stage_observations(poses, obs)
                fl.update_map()
            for grid in (N.GRID_MASTER, N.GRID_OBSTACLE):
                assert np.array_equal(a.download(grid), twin.download(grid)), (cyc, grid)
            assert np.array_equal(a.bounds(), twin.bounds()), cyc
            if cyc == 2:
                break
            grid, value = ((N.GRID_OBSTACLE, 0), (N.GRID_MASTER, 254))[cyc]
            assert a.set_polygon_cost(grid, poly, value) == [True] * nI
            g = twin.download(grid)
            for i in range(nI):
                gi = np.ascontiguousarray(g[i])
                assert orc.lib().orc_polygon_fill(gi, n, n, RES, 0.0, 0.0, np.ascontiguousarray(poly[i]), len(poly[i]), value) == 1
                g[i] = gi
            twin.upload(grid, g)
            assert np.array_equal(a.download(grid), g), "the polygon write differs from the oracle's"
    finally:
        for fl in fleets:
            fl.close()
