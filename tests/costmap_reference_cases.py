"""The costmap reference fixture (tests/golden/g17_costmap_reference.npz): its cases, the harness's input / output layouts, the
exact-distance inflation specification and a reader.

build_cases() is what tools/make_costmap_goldens.py feeds tools/costmap_reference_harness.cpp; load() / case() are what the tests read
the committed file with.  No oracle, no library and no reference tree in here.

A case is a dict: name, size_x, size_y, res, ox, oy, rolling, track_unknown, static (None or a dict), obstacle (None or a dict),
inflation (None or a dict), fp (k, 2), cycles: a list of dict(pose, fp (None: unchanged), inflation (None: unchanged), obs: a list of
dict(points (n, 3) float32, origin, obstacle_range, raytrace_range, marking, clearing)).

Every resolution is RES, the float32 nearest to 0.05 as a double: nav_msgs/MapMetaData carries a float32, and StaticLayer::incomingMap
resizes a fixed-size costmap whose resolution differs from the map's."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_costmap_reference.npz")
FREE, INSCRIBED, LETHAL, NOINFO = 0, 253, 254, 255
RES = float(np.float32(0.05))
FP_SQUARE = [[0.2, 0.2], [0.2, -0.2], [-0.2, -0.2], [-0.2, 0.2]]        # inscribed radius 0.2
FP_NARROW = [[0.3, 0.15], [0.3, -0.15], [-0.3, -0.15], [-0.3, 0.15]]    # inscribed radius 0.15
STATIC_DEFAULTS = dict(track_unknown_space=True, use_maximum=False, trinary=True, lethal_threshold=100, unknown_cost_value=-1)
OBSTACLE_DEFAULTS = dict(voxel=False, combination_method=1, footprint_clearing=True, max_obstacle_height=2.0, z_voxels=10, origin_z=0.0,
                         z_resolution=0.2, unknown_threshold=15, mark_threshold=0)


def radius_for(cells):
    """an inflation radius whose cell radius ceil(radius / RES) is `cells`"""
    return (cells - 0.5) * 0.05


# ------------------------------------------------------------------------------------------------ inputs
def _pts(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3).astype(np.float32))


def _obs(points, origin, obstacle_range=2.5, raytrace_range=3.0, marking=True, clearing=True):
    return dict(points=_pts(points), origin=tuple(float(v) for v in origin), obstacle_range=float(obstacle_range),
                raytrace_range=float(raytrace_range), marking=bool(marking), clearing=bool(clearing))


def _scan(rs, cx, cy, n, rmin, rmax, z=0.3, zspread=0.0):
    a = rs.uniform(-np.pi, np.pi, n)
    r = rs.uniform(rmin, rmax, n)
    z = z + rs.uniform(-zspread, zspread, n)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a), z], 1)


def _cycle(pose, obs=(), fp=None, inflation=None):
    return dict(pose=tuple(float(v) for v in pose), obs=list(obs), fp=fp, inflation=inflation)


def _case(name, size_x, size_y, cycles, ox=0.0, oy=0.0, rolling=False, track_unknown=False, static=None, obstacle=None, inflation=None,
          fp=FP_SQUARE):
    c = dict(name=name, size_x=size_x, size_y=size_y, res=RES, ox=float(ox), oy=float(oy), rolling=rolling, track_unknown=track_unknown,
             static=None if static is None else dict(STATIC_DEFAULTS, **static),
             obstacle=None if obstacle is None else dict(OBSTACLE_DEFAULTS, **obstacle),
             inflation=inflation, fp=[list(map(float, p)) for p in fp], cycles=cycles)
    assert 48 <= size_x <= 130 and 48 <= size_y <= 130 and 1 <= len(cycles) <= 4, name
    if c["static"] is not None:
        s = c["static"]
        s.setdefault("res", RES)
        s.setdefault("ox", c["ox"])
        s.setdefault("oy", c["oy"])
        s["occ"] = np.ascontiguousarray(s["occ"], np.int8)
        assert rolling or s["occ"].shape == (size_y, size_x)
    return c


def grey_map(rs, size_x, size_y):
    """an occupancy grid that holds every byte from -128 to 127, most of it free"""
    occ = np.zeros((size_y, size_x), np.int8)
    some = rs.random_sample(occ.shape) < 0.12
    occ[some] = rs.randint(-128, 128, int(some.sum())).astype(np.int8)
    flat = occ.reshape(-1)
    at = rs.choice(flat.size, 256, replace=False)
    flat[at] = np.arange(-128, 128).astype(np.int8)
    return occ


def _border_seeds(occ, value=100):
    """lethal cells in the four corners and on the four borders, an unknown cell beside some of them"""
    sy, sx = occ.shape
    for y, x in ((0, 0), (0, sx - 1), (sy - 1, 0), (sy - 1, sx - 1), (0, sx // 3), (sy - 1, sx // 2), (sy // 3, 0), (sy // 2, sx - 1)):
        occ[y, x] = value
    for y, x in ((1, 0), (sy - 1, sx // 2 + 1), (sy // 2 - 1, sx - 1), (1, sx // 3)):
        occ[y, x] = -1
    return occ


def build_cases():
    cases = []
    W = 2.5  # obstacle_range of the scans
    # ---------------------------------------------------------------- ObstacleLayer, fixed window
    rs = np.random.RandomState(1701)
    ox, oy, nx, ny = -1.0, 0.5, 96, 80
    ex, ey = ox + nx * RES, oy + ny * RES
    sx_, sy_ = 1.5, 2.5  # sensor, in the map; 1.5 - ox = 2.5 m from the left edge, 2.3 m from the right
    special = [
        [sx_ + 1.5, sy_ + 2.0, 0.5],    # exactly at obstacle_range 2.5 (3-4-5 triangle, every term a binary fraction): not marked
        [sx_ - 2.5, sy_, 0.5],          # exactly at it along an axis: not marked (lands on the left edge cell)
        [sx_ + 1.5, sy_ + 1.96875, 0.5],  # just inside
        [sx_ + 2.0, sy_ + 1.75, 0.5],   # beyond
        [sx_ + 0.5, sy_ + 0.5, 2.25],   # above max_obstacle_height (and far in z)
        [sx_ + 0.4, sy_ - 0.3, 2.0],    # exactly max_obstacle_height: kept (the test is >)
        [ox - 0.3, sy_ + 0.2, 0.5], [ex + 0.4, sy_ - 0.1, 0.5], [sx_ + 0.1, oy - 0.6, 0.5], [sx_ - 0.2, ey + 0.2, 0.5],  # off the map, each side
        [ox - 0.5, oy - 0.7, 0.5], [ex + 0.6, ey + 0.3, 0.5], [ex + 0.2, oy - 0.2, 0.5], [ox - 0.1, ey + 0.9, 0.5],      # through the corners
        [sx_, sy_, 0.5],                # a zero-length ray
        [sx_ + 3.0, sy_, 0.5],          # exactly at raytrace_range 3.0 along an axis (off the map: clipped first)
        [sx_ + 1.8, sy_ - 1.0, 0.5], [sx_ - 1.0, sy_ + 1.25, 0.5],
    ]
    scan0 = np.concatenate([special, _scan(rs, sx_, sy_, 150, 0.4, 3.4, 0.5, 0.4)])
    far = _scan(rs, sx_, sy_, 40, 4.0, 9.0)  # endpoints far beyond the map: every edge and corner
    near = _scan(rs, sx_ + 0.1, sy_, 12, 0.5, 0.8)
    cases.append(_case("obstacle_fixed", nx, ny, ox=ox, oy=oy, obstacle=dict(), inflation=dict(radius=radius_for(11), scaling=10.0), cycles=[
        _cycle((sx_, sy_, 0.3), [_obs(scan0, (sx_, sy_, 0.5), W, 3.0)]),
        _cycle((sx_ + 0.1, sy_, 0.5), [_obs(_scan(rs, sx_, sy_, 60, 0.5, 2.4), (sx_ + 0.1, sy_, 0.5), W, 3.0, True, False),       # marks only
                                      _obs(far, (sx_ + 0.1, sy_ + 0.05, 0.5), W, 100.0, False, True)]),                         # clears only
        _cycle((sx_ + 0.1, sy_, 0.5), [_obs(near, (sx_ + 0.1, sy_, 0.5), W, 1.0)]),   # little new data: the box is still the one before
        _cycle((sx_ + 0.1, sy_, 0.5), [_obs(near[::2] + np.float32(0.05), (sx_ + 0.1, sy_, 0.5), W, 1.0)]),                      # a smaller box
    ]))
    # the sensor off the map (its rays are skipped, its points still mark); raytrace_range inside the map; a footprint off the map
    rs = np.random.RandomState(1702)
    nx, ny = 48, 52
    c = (nx * RES / 2, ny * RES / 2)
    cases.append(_case("obstacle_small_map", nx, ny, obstacle=dict(footprint_clearing=True), track_unknown=True,
                       inflation=dict(radius=radius_for(5), scaling=10.0), cycles=[
        _cycle((c[0], c[1], 0.0), [_obs(_scan(rs, c[0], c[1], 90, 0.3, 1.2), (-0.4, c[1], 0.3), 4.0, 3.0),      # sensor off the map
                                  _obs(_scan(rs, c[0], c[1], 90, 0.3, 4.0), (c[0], c[1], 0.3), 1.1, 0.8)]),    # range cuts, rays leave everywhere
        _cycle((0.1, c[1], 0.7), [_obs(_scan(rs, c[0], c[1], 50, 0.3, 1.0), (c[0] + 0.02, c[1], 0.3), 1.1, 100.0)]),  # a vertex off the map
        _cycle((c[0], ny * RES - 0.15, 2.0), [_obs(_scan(rs, c[0], c[1], 50, 0.2, 3.0), (c[0], c[1] - 0.3, 0.3), 2.0, 0.55)]),
    ]))
    # ---------------------------------------------------------------- static under obstacle: both combination methods, both merges
    rs = np.random.RandomState(1703)
    nx, ny = 130, 70
    occ = _border_seeds(grey_map(rs, nx, ny))
    c = (nx * RES / 2, ny * RES / 2)
    cyc = [_cycle((c[0], c[1], 0.2), [_obs(_scan(rs, c[0], c[1], 160, 0.3, 3.2), (c[0], c[1], 0.4), W, 3.0)]),
           _cycle((c[0] + 0.3, c[1], 0.4), [_obs(_scan(rs, c[0], c[1], 120, 0.3, 3.2), (c[0] + 0.3, c[1], 0.4), W, 3.0)])]
    cases.append(_case("static_grey_overwrite", nx, ny, cyc, track_unknown=True, static=dict(occ=occ, trinary=False),
                       obstacle=dict(combination_method=0, footprint_clearing=False), inflation=dict(radius=radius_for(11), scaling=3.0)))
    cases.append(_case("static_grey_max", nx, ny, cyc, track_unknown=True, static=dict(occ=occ, trinary=False, use_maximum=True),
                       obstacle=dict(combination_method=1), inflation=dict(radius=radius_for(11), scaling=3.0)))
    cases.append(_case("static_trinary_overwrite_no_unknown", nx, ny, cyc, track_unknown=False,
                       static=dict(occ=occ, trinary=True, track_unknown_space=False), obstacle=dict(combination_method=0)))
    # ---------------------------------------------------------------- static as the only layer
    rs = np.random.RandomState(1704)
    occ = grey_map(rs, 64, 48)
    one = [_cycle((1.0, 1.0, 0.0)), _cycle((1.0, 1.0, 0.0))]  # the second cycle has no new data: an empty box
    cases.append(_case("static_only_trinary", 64, 48, one, track_unknown=True, static=dict(occ=occ)))
    cases.append(_case("static_only_scaled", 64, 48, one, track_unknown=True,
                       static=dict(occ=occ, trinary=False, lethal_threshold=65, unknown_cost_value=77)))
    cases.append(_case("static_only_scaled_no_unknown_max", 64, 48, one, track_unknown=False,
                       static=dict(occ=occ, trinary=False, lethal_threshold=65, unknown_cost_value=77, track_unknown_space=False, use_maximum=True)))
    # ---------------------------------------------------------------- inflation: radii, scaling, borders, partial boxes, the previous box
    rs = np.random.RandomState(1705)
    nx, ny = 130, 96
    occ = _border_seeds(grey_map(rs, nx, ny))
    occ[rs.random_sample(occ.shape) < 0.004] = 100
    c = (nx * RES / 2, ny * RES / 2)
    cases.append(_case("inflation_r14_grey", nx, ny, track_unknown=True, static=dict(occ=occ, trinary=False), obstacle=dict(),
                       inflation=dict(radius=radius_for(14), scaling=3.0), cycles=[
        _cycle((c[0], c[1], 0.0), [_obs(_scan(rs, c[0], c[1], 60, 0.4, 2.4), (c[0], c[1], 0.4), W, 3.0)]),
        _cycle((0.4, 0.4, 0.0), [_obs(_scan(rs, 0.4, 0.4, 40, 0.3, 0.6), (0.4, 0.4, 0.4), W, 0.5)]),   # with the box before: the whole map
        _cycle((0.4, 0.4, 0.0), [_obs(_scan(rs, 0.4, 0.4, 40, 0.3, 0.6), (0.4, 0.4, 0.4), W, 0.5)]),   # the left and bottom borders clip the box
        _cycle((c[0], c[1], 0.0), [_obs(_scan(rs, c[0], c[1], 10, 0.3, 0.4), (c[0], c[1], 0.4), W, 0.3)]),  # the box before and a small one
    ]))
    rs = np.random.RandomState(1706)
    nx, ny = 64, 64
    occ = np.zeros((ny, nx), np.int8)
    occ[rs.random_sample(occ.shape) < 0.01] = 100
    occ[rs.random_sample(occ.shape) < 0.03] = -1
    _border_seeds(occ)
    c = (nx * RES / 2, ny * RES / 2)
    far_corner = (nx * RES - 0.4, ny * RES - 0.4, 0.0)
    for r, scaling in ((5, 10.0), (1, 10.0)):
        cases.append(_case(f"inflation_r{r}", nx, ny, track_unknown=True, static=dict(occ=occ), obstacle=dict(),
                           inflation=dict(radius=radius_for(r), scaling=scaling), cycles=[
            _cycle((c[0], c[1], 0.0), [_obs(_scan(rs, c[0], c[1], 40, 0.4, 1.4), (c[0], c[1], 0.4), W, 3.0)]),
            _cycle(far_corner, [_obs(_scan(rs, far_corner[0], far_corner[1], 10, 0.3, 0.6), (far_corner[0], far_corner[1], 0.4), W, 0.5)]),
            _cycle(far_corner, [_obs(_scan(rs, far_corner[0], far_corner[1], 10, 0.3, 0.6), (far_corner[0], far_corner[1], 0.4), W, 0.5)]),  # right, top clip
            _cycle((c[0], c[1], 0.0), [_obs(_scan(rs, c[0], c[1], 10, 0.4, 0.6), (c[0], c[1], 0.4), W, 3.0)], fp=FP_NARROW),  # reinflation
        ]))
    # one lethal cell per inflation disc: the walk and the exact distance agree (no two sources compete for a cell)
    occ = np.zeros((ny, nx), np.int8)
    for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (30, 37)):
        occ[y, x] = 100
    cases.append(_case("inflation_lone_seeds", nx, ny, [_cycle((1.0, 1.0, 0.0))], static=dict(occ=occ),
                       inflation=dict(radius=radius_for(14), scaling=10.0)))
    # ---------------------------------------------------------------- rolling windows, 2-D and voxel
    for kind in ("2d", "voxel"):
        vox = dict(voxel=True) if kind == "voxel" else dict()
        for tag, moves in (("a", [(0.0, 0.0), (0.43, 0.31), (-0.62, -0.47), (0.012, 0.02)]),          # start; + +; - -; within a cell
                           ("b", [(0.0, 0.0), (0.0, 0.0), (0.33, -0.52), (9.0, -7.0)])):              # start; no move; + -; out of the window
            rs = np.random.RandomState(1710 + len(cases))
            nx, ny = (80, 60) if tag == "a" else (66, 72)
            x, y = 5.0, 4.0
            cyc = []
            for k, (dx, dy) in enumerate(moves):
                x, y = x + dx, y + dy
                cyc.append(_cycle((x, y, 0.3 * k), [_obs(_scan(rs, x, y, 70, 0.4, 2.2, 0.5, 0.45 if vox else 0.0), (x, y, 0.5), W, 3.0)]))
            cases.append(_case(f"rolling_{kind}_{tag}", nx, ny, cyc, rolling=True, track_unknown=(tag == "b"), obstacle=dict(vox),
                               inflation=dict(radius=radius_for(11), scaling=10.0)))
    # a static map larger than the window and offset from it, read through the identity transform
    rs = np.random.RandomState(1720)
    occ = grey_map(rs, 120, 100)
    occ[40:43, 10:100] = 100
    x, y = 6.0, 5.5
    cyc = [_cycle((x + 0.4 * k, y - 0.3 * k, 0.1), [_obs(_scan(rs, x + 0.4 * k, y - 0.3 * k, 50, 0.4, 2.0), (x + 0.4 * k, y - 0.3 * k, 0.4), W, 3.0)])
           for k in range(3)]
    cyc.append(_cycle((3.2, 4.2, 0.0), []))  # the window hangs over the static map's corner
    for name, st in (("rolling_static", dict()), ("rolling_static_max_scaled", dict(use_maximum=True, trinary=False, track_unknown_space=False))):
        cases.append(_case(name, 64, 48, cyc, rolling=True, track_unknown=True, static=dict(occ=occ, res=RES, ox=3.0, oy=4.0, **st),
                           obstacle=dict(), inflation=dict(radius=radius_for(5), scaling=10.0)))
    # ---------------------------------------------------------------- VoxelLayer, fixed window
    for k, (name, v, top) in enumerate((
            ("voxel_z10", dict(z_voxels=10, origin_z=0.0, z_resolution=0.2, unknown_threshold=15, mark_threshold=0), 2.0),
            ("voxel_z16_neg_origin", dict(z_voxels=16, origin_z=-0.3, z_resolution=0.1, unknown_threshold=4, mark_threshold=1), 1.3),
            ("voxel_z5", dict(z_voxels=5, origin_z=0.0, z_resolution=0.25, unknown_threshold=0, mark_threshold=0), 1.25),
            ("voxel_z1", dict(z_voxels=1, origin_z=-0.3, z_resolution=0.2, unknown_threshold=15, mark_threshold=0), -0.1))):
        rs = np.random.RandomState(1730 + k)
        nx, ny = (100, 64) if k % 2 == 0 else (57, 75)
        c = (nx * RES / 2, ny * RES / 2)
        oz = v["origin_z"]
        sz = min(0.45, (oz + top) / 2) if top > oz + 0.3 else oz + 0.1  # the sensor, inside the grid
        cyc = []
        for n in range(3):
            # points through the grid's height, above it (below and above max_obstacle_height 2.0) and below origin_z
            pts = np.concatenate([_scan(rs, c[0], c[1], 90, 0.3, 3.2, (oz + top) / 2, (top - oz) / 2 + 0.15),
                                  _scan(rs, c[0], c[1], 12, 0.5, 2.0, 2.3, 0.2), _scan(rs, c[0], c[1], 12, 0.5, 2.0, oz - 0.25, 0.2),
                                  [[c[0] + 0.8 * np.cos(a), c[1] + 0.8 * np.sin(a), z] for a in np.arange(8) * 0.7 + n     # stacked points: columns
                                   for z in np.linspace(oz + 0.02, top - 0.02, 4)],                                      # with several marked voxels
                                  [[c[0], c[1], sz]]])
            cyc.append(_cycle((c[0] + 0.05 * n, c[1], 0.4 * n), [_obs(pts, (c[0] + 0.03 * n, c[1], sz), W, 3.0)]))
        cyc[1]["obs"].append(_obs(_scan(rs, c[0], c[1], 30, 3.5, 8.0, 0.3, 1.5), (c[0], c[1] + 0.1, sz), W, 100.0, False, True))
        cases.append(_case(name, nx, ny, cyc, track_unknown=(k != 0), obstacle=dict(voxel=True, **v),
                           inflation=dict(radius=radius_for(5), scaling=10.0)))
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


# ------------------------------------------------------------------------------------------------ harness layouts
def encode_input(c):
    d = [c["size_x"], c["size_y"], c["res"], c["ox"], c["oy"], int(c["rolling"]), int(c["track_unknown"])]
    s = c["static"]
    if s is None:
        d += [0] * 11
    else:
        sy, sx = s["occ"].shape
        d += [1, sx, sy, s["res"], s["ox"], s["oy"], int(s["track_unknown_space"]), int(s["use_maximum"]), int(s["trinary"]),
              s["lethal_threshold"], s["unknown_cost_value"]]
    o = c["obstacle"]
    if o is None:
        d += [0] * 9
    else:
        d += [2 if o["voxel"] else 1, o["combination_method"], int(o["footprint_clearing"]), o["max_obstacle_height"], o["z_voxels"],
              o["origin_z"], o["z_resolution"], o["unknown_threshold"], o["mark_threshold"]]
    i = c["inflation"]
    d += [0, 0, 0] if i is None else [1, i["radius"], i["scaling"]]
    d += [len(c["fp"])] + [v for p in c["fp"] for v in p]
    parts = [np.asarray(d, np.float64)]
    if s is not None:
        parts.append(s["occ"].reshape(-1).astype(np.float64))
    parts.append(np.asarray([len(c["cycles"])], np.float64))
    for cyc in c["cycles"]:
        d = list(cyc["pose"])
        fp = cyc["fp"] or []
        d += [len(fp)] + [float(v) for p in fp for v in p]
        i = cyc["inflation"]
        d += [0, 0, 0] if i is None else [1, i["radius"], i["scaling"]]
        d += [len(cyc["obs"])]
        parts.append(np.asarray(d, np.float64))
        for ob in cyc["obs"]:
            parts.append(np.asarray(list(ob["origin"]) + [ob["obstacle_range"], ob["raytrace_range"], int(ob["marking"]), int(ob["clearing"]),
                                                          len(ob["points"])], np.float64))
            parts.append(ob["points"].reshape(-1).astype(np.float64))
    return np.concatenate(parts)


def decode_input(d):
    """the case dict back from encode_input's doubles"""
    d = np.asarray(d, np.float64)
    at = [0]

    def take(n=1):
        v = d[at[0]:at[0] + n]
        at[0] += n
        return v

    size_x, size_y, res, ox, oy, rolling, track_unknown = take(7)
    c = dict(size_x=int(size_x), size_y=int(size_y), res=float(res), ox=float(ox), oy=float(oy), rolling=bool(rolling), track_unknown=bool(track_unknown))
    s = take(11)
    c["static"] = None if not s[0] else dict(res=float(s[3]), ox=float(s[4]), oy=float(s[5]), track_unknown_space=bool(s[6]), use_maximum=bool(s[7]),
                                             trinary=bool(s[8]), lethal_threshold=int(s[9]), unknown_cost_value=int(s[10]))
    o = take(9)
    c["obstacle"] = None if not o[0] else dict(voxel=o[0] == 2, combination_method=int(o[1]), footprint_clearing=bool(o[2]), max_obstacle_height=float(o[3]),
                                               z_voxels=int(o[4]), origin_z=float(o[5]), z_resolution=float(o[6]), unknown_threshold=int(o[7]),
                                               mark_threshold=int(o[8]))
    i = take(3)
    c["inflation"] = None if not i[0] else dict(radius=float(i[1]), scaling=float(i[2]))
    c["fp"] = take(2 * int(take()[0])).reshape(-1, 2).tolist()
    if c["static"] is not None:
        c["static"]["occ"] = take(int(s[1]) * int(s[2])).astype(np.int8).reshape(int(s[2]), int(s[1]))
    c["cycles"] = []
    for _ in range(int(take()[0])):
        pose = tuple(take(3).tolist())
        fp = take(2 * int(take()[0])).reshape(-1, 2).tolist() or None
        i = take(3)
        obs = []
        for _ in range(int(take()[0])):
            h = take(8)
            obs.append(dict(origin=tuple(h[0:3].tolist()), obstacle_range=float(h[3]), raytrace_range=float(h[4]), marking=bool(h[5]), clearing=bool(h[6]),
                            points=take(3 * int(h[7])).astype(np.float32).reshape(-1, 3)))
        c["cycles"].append(dict(pose=pose, fp=fp, inflation=None if not i[0] else dict(radius=float(i[1]), scaling=float(i[2])), obs=obs))
    assert at[0] == len(d)
    return c


def cell_radius(c, upto):
    """the inflation radius in cells during cycle `upto`: Costmap2D::cellDistance of the radius last set"""
    i = c["inflation"]
    for cyc in c["cycles"][:upto + 1]:
        i = cyc["inflation"] or i
    return int(max(0.0, math.ceil(i["radius"] / c["res"])))


def stages(c):
    """the layers of a case in plugin order"""
    return [k for k in ("static", "obstacle", "inflation") if c[k] is not None]


def decode_output(raw, c):
    """the harness's bytes for case c -> a list of per-cycle dicts"""
    raw = np.frombuffer(bytes(raw), np.uint8)
    n = c["size_x"] * c["size_y"]
    shape = (c["size_y"], c["size_x"])
    at = 0
    out = []
    for k in range(len(c["cycles"])):
        r = dict(origin=raw[at:at + 16].view(np.float64).copy(), box=raw[at + 16:at + 32].view(np.int32).copy())
        at += 32
        if c["obstacle"] is not None:
            r["layer"] = raw[at:at + n].reshape(shape).copy()
            at += n
            if c["obstacle"]["voxel"]:
                r["voxels"] = raw[at:at + 4 * n].view(np.uint32).reshape(shape).copy()
                at += 4 * n
        for st in stages(c):
            r["master_" + st] = raw[at:at + n].reshape(shape).copy()
            at += n
        if c["inflation"] is not None:
            R = int(raw[at:at + 4].view(np.int32)[0])
            assert R == cell_radius(c, k), (c["name"], k, R)
            r["inscribed"] = raw[at + 4:at + 12].view(np.float64).copy()[0]
            r["cost_table"] = raw[at + 12:at + 12 + (R + 2) ** 2].reshape(R + 2, R + 2).copy()
            at += 12 + (R + 2) ** 2
        out.append(r)
    assert at == len(raw), (c["name"], at, len(raw))
    return out


# ------------------------------------------------------------------------------------------------ the exact-distance specification
def inflate_exact(master, box, table):
    """The order-independent inflation: every cell within the radius of a lethal cell of the grown, clipped box takes the cost
    table[|dx|, |dy|] of the nearest one, written with InflationLayer::updateCosts' rule (an unknown cell takes inscribed and lethal
    costs only, any other cell the maximum).  table is the reference's computeCost(hypot(i, j)), i, j <= R + 1; box = x0, xn, y0, yn."""
    sy, sx = master.shape
    R = table.shape[0] - 2
    x0, xn, y0, yn = (int(v) for v in box)
    x0, y0, xn, yn = max(0, x0 - R), max(0, y0 - R), min(sx, xn + R), min(sy, yn + R)
    seeds = np.zeros(master.shape, bool)
    seeds[y0:yn, x0:xn] = master[y0:yn, x0:xn] == LETHAL
    far = (R + 2) ** 2 * 2
    d2 = np.full(master.shape, far, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx * dx + dy * dy > R * R:
                continue
            ys, yd = slice(max(0, -dy), min(sy, sy - dy)), slice(max(0, dy), min(sy, sy + dy))
            xs, xd = slice(max(0, -dx), min(sx, sx - dx)), slice(max(0, dx), min(sx, sx + dx))
            hit = seeds[ys, xs]
            d2[yd, xd] = np.where(hit, np.minimum(d2[yd, xd], dx * dx + dy * dy), d2[yd, xd])
    by_d2 = np.zeros(far + 1, np.uint8)
    for i in range(R + 1):
        for j in range(R + 1):
            if i * i + j * j <= R * R:
                by_d2[i * i + j * j] = table[i, j]
    reached = d2 < far
    cost = by_d2[np.minimum(d2, far)]
    out = master.copy()
    take = reached & (master == NOINFO) & (cost >= INSCRIBED)
    out[take] = cost[take]
    rest = reached & ~((master == NOINFO) & (cost >= INSCRIBED))
    out[rest] = np.maximum(master[rest], cost[rest])
    return out


def shift_window(grid, prev_origin, origin, res, fill):
    """a rolling window's grid after its origin moved by whole cells: what stays in the window keeps its world position"""
    ox, oy = (int(v) for v in np.rint((np.asarray(origin) - np.asarray(prev_origin)) / res))
    sy, sx = grid.shape
    out = np.full_like(grid, fill)
    ys, yd = slice(max(0, oy), min(sy, sy + oy)), slice(max(0, -oy), min(sy, sy - oy))
    xs, xd = slice(max(0, ox), min(sx, sx + ox)), slice(max(0, -ox), min(sx, sx - ox))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = grid[ys, xs]
    return out


def exact_masters(c, recs):
    """The master grids of a costmap whose inflation layer follows the specification in every cycle.  Inside a cycle's box the grid in
    front of the inflation layer is the reference's (recs[k]["master_<layer>"]: it does not depend on earlier inflation); outside the
    box it is what the cycle before left, moved with a rolling window.  Asserts that the reference's own grids obey that same rule."""
    before = "master_" + stages(c)[-2]
    fill = NOINFO if c["track_unknown"] else FREE
    out = []
    for k, r in enumerate(recs):
        pre = r[before].copy()
        x0, xn, y0, yn = (int(v) for v in r["box"])
        outside = np.ones(pre.shape, bool)
        if xn >= x0 and yn >= y0:
            outside[y0:yn, x0:xn] = False
        if k:
            carried_ref, carried = recs[k - 1].get("master_inflation", recs[k - 1].get("master")), out[-1]
            if c["rolling"]:
                carried_ref = shift_window(carried_ref, recs[k - 1]["origin"], r["origin"], c["res"], fill)
                carried = shift_window(carried, recs[k - 1]["origin"], r["origin"], c["res"], fill)
            assert np.array_equal(pre[outside], carried_ref[outside]), (c["name"], k)
            pre[outside] = carried[outside]
        else:
            assert not outside.any(), c["name"]
        out.append(inflate_exact(pre, r["box"], r["cost_table"]) if not outside.all() else pre)
    return out


# ------------------------------------------------------------------------------------------------ the committed file
def load():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["meta"]))


def case(g, meta, name):
    """(case dict, per-cycle records) of a case of the committed fixture.  A record holds origin, box, layer / voxels (where stored),
    master_static / master_obstacle (where layers stack), master (the final grid) and, with an inflation layer, inscribed (the footprint's inscribed radius), cost_table and
    master_exact (the specification built from cost_table)."""
    c = decode_input(g[name + "_in"])
    c["name"] = name
    out = []
    for k in range(len(c["cycles"])):
        r = dict(origin=g[name + "_origin"][k], box=g[name + "_box"][k], master=g[name + "_master"][k])
        for key in ("layer", "master_static", "master_obstacle", "master_exact", "cost_table", "inscribed"):
            if f"{name}_{key}" in g.files:
                r[key] = g[f"{name}_{key}"][k]
        if f"{name}_voxels" in g.files:
            cycles = meta["voxel_cycles"][name]
            if k in cycles:
                r["voxels"] = g[name + "_voxels"][cycles.index(k)]
        out.append(r)
    return c, out
