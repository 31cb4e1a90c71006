"""Restatements, written for the voxel-export tests, of the reference code that navgpu_voxel_points and
navgpu_voxel_clearing_endpoints replace - shared by tests/test_voxel_export_host.py (which pins them on the CPU) and
tests/test_gpu_voxel_export.py (which compares the device against them):

  get_voxel / voxel_points  VoxelGrid::getVoxel (voxel_grid/include/voxel_grid/voxel_grid.h:183-206) under the loops of
                            costmap_2d_cloud.cpp:85-122, with mapToWorld3D (:36-42)
  clearing_endpoints        VoxelLayer::raytraceFreespace (costmap_2d/plugins/voxel_layer.cpp:266-381) up to the point it pushes
                            into clearing_endpoints_, in plain fp64, statement by statement
  clear_voxel_line          VoxelGrid::raytraceLine + bresenham3D with ClearVoxel (voxel_grid.h:226-308), to carry the endpoints
                            to the oracle's voxel grid
Nothing here reads the product."""
import numpy as np

FREE, UNKNOWN, MARKED = 0, 1, 2  # voxel_grid::VoxelStatus
f64 = np.float64


def get_voxel(cols, z_voxels):
    """status of every (y, x, z < z_voxels): numBits(data & full_mask) - 2 marked, 1 unknown, 0 free"""
    cols = np.asarray(cols, np.uint32)
    z = np.arange(z_voxels, dtype=np.uint32)
    lo = (cols[..., None] >> z) & np.uint32(1)
    hi = (cols[..., None] >> (z + np.uint32(16))) & np.uint32(1)
    return (lo + hi).astype(np.uint8)


def voxel_points(cols, status, z_voxels, ox, oy, res, origin_z, z_res, as_double):
    """the cloud of one status in the loop order y, x, z (np.nonzero walks the (y, x, z) array in C order)"""
    my, mx, mz = np.nonzero(get_voxel(cols, z_voxels) == status)
    wx = f64(ox) + (mx.astype(np.float64) + 0.5) * f64(res)
    wy = f64(oy) + (my.astype(np.float64) + 0.5) * f64(res)
    wz = f64(origin_z) + (mz.astype(np.float64) + 0.5) * f64(z_res)
    xyz = np.stack([wx, wy, wz], axis=1)
    return xyz if as_double else xyz.astype(np.float32)  # Point32: float fields


class Geometry:
    """what VoxelLayer holds: Costmap2D origin / resolution / size, origin_z_, z_resolution_, size_z_, max_obstacle_height_"""

    def __init__(self, ox, oy, res, nx, ny, origin_z, z_res, z_voxels, max_obstacle_height):
        self.ox, self.oy, self.res = f64(ox), f64(oy), f64(res)
        self.nx, self.ny, self.size_z = nx, ny, z_voxels
        self.origin_z, self.z_res, self.max_h = f64(origin_z), f64(z_res), f64(max_obstacle_height)


def _min(a, b):  # std::min
    return b if b < a else a


def _max(a, b):  # std::max
    return b if a < b else a


def world_to_map_3d_float(g, wx, wy, wz):
    """voxel_layer.h:107-118 -> (ok, mx, my, mz, margin): margin = the smallest distance, in cells, of a comparison it
    evaluated from its threshold"""
    margin = min(abs(wx - g.ox) / g.res, abs(wy - g.oy) / g.res, abs(wz - g.origin_z) / g.z_res)
    if wx < g.ox or wy < g.oy or wz < g.origin_z:
        return False, None, None, None, margin
    mx = (wx - g.ox) / g.res
    my = (wy - g.oy) / g.res
    mz = (wz - g.origin_z) / g.z_res
    margin = min(margin, abs(mx - g.nx), abs(my - g.ny), abs(mz - g.size_z))
    return bool(mx < g.nx and my < g.ny and mz < g.size_z), mx, my, mz, margin


def clearing_endpoints(g, points, origin):
    """One clearing observation -> dict(sensor = its origin in cells or None, kept = indices of the points that yield an
    endpoint, ends = their (wpx, wpy, wpz) doubles, cells = their (point_x, point_y, point_z), margin = per point of the cloud
    the decision margin of the final worldToMap3DFloat, on_threshold = per point whether the clip itself put a coordinate onto
    the threshold it is then compared with (:325, :331, :335: the floor and the two lower map edges))."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    out = dict(sensor=None, kept=[], ends=[], cells=[], margin=np.full(len(pts), np.inf), on_threshold=np.zeros(len(pts), bool))
    if len(pts) == 0:  # :269-270
        return out
    ox, oy, oz = f64(origin[0]), f64(origin[1]), f64(origin[2])
    ok, sx, sy, sz, _ = world_to_map_3d_float(g, ox, oy, oz)
    if not ok:  # :277-284
        return out
    out["sensor"] = (sx, sy, sz)
    # getSizeInMetersX(): (size_x_ - 1 + 0.5) * resolution_ (costmap_2d.cpp:448-456)
    map_end_x = g.ox + (g.nx - 1 + 0.5) * g.res
    map_end_y = g.oy + (g.ny - 1 + 0.5) * g.res
    with np.errstate(all="ignore"):
        for i in range(len(pts)):
            wpx, wpy, wpz = f64(pts[i, 0]), f64(pts[i, 1]), f64(pts[i, 2])
            distance = np.sqrt((wpx - ox) * (wpx - ox) + (wpy - oy) * (wpy - oy) + (wpz - oz) * (wpz - oz))
            scaling_fact = f64(1.0)
            scaling_fact = _max(_min(scaling_fact, (distance - 2 * g.res) / distance), f64(0.0))
            wpx = scaling_fact * (wpx - ox) + ox
            wpy = scaling_fact * (wpy - oy) + oy
            wpz = scaling_fact * (wpz - oz) + oz
            a = wpx - ox
            b = wpy - oy
            c = wpz - oz
            t = f64(1.0)
            hit = [False, False, False]  # which lower threshold decided t last
            if wpz > g.max_h:
                t = _max(f64(0.0), _min(t, (g.max_h - 0.01 - oz) / c))
            elif wpz < g.origin_z:
                t = _min(t, (g.origin_z - oz) / c)
                hit = [False, False, True]
            if wpx < g.ox:
                t2 = _min(t, (g.ox - ox) / a)
                if t2 != t:
                    hit = [True, False, False]
                t = t2
            if wpy < g.oy:
                t2 = _min(t, (g.oy - oy) / b)
                if t2 != t:
                    hit = [False, True, False]
                t = t2
            if wpx > map_end_x:
                t2 = _min(t, (map_end_x - ox) / a)
                if t2 != t:
                    hit = [False, False, False]
                t = t2
            if wpy > map_end_y:
                t2 = _min(t, (map_end_y - oy) / b)
                if t2 != t:
                    hit = [False, False, False]
                t = t2
            wpx = ox + a * t
            wpy = oy + b * t
            wpz = oz + c * t
            ok, px, py, pz, margin = world_to_map_3d_float(g, wpx, wpy, wpz)
            out["margin"][i] = margin
            out["on_threshold"][i] = any(hit)
            if ok:  # :353
                out["kept"].append(i)
                out["ends"].append((wpx, wpy, wpz))
                out["cells"].append((px, py, pz))
    return out


def clear_voxel_line(cols, nx, x0, y0, z0, x1, y1, z1, max_length=0xFFFFFFFF):
    """VoxelGrid::raytraceLine(ClearVoxel, ...) on the flat uint32 column array `cols` (modified in place)"""
    dx, dy, dz = int(x1) - int(x0), int(y1) - int(y0), int(z1) - int(z0)
    abs_dx, abs_dy, abs_dz = abs(dx), abs(dy), abs(dz)
    sign = lambda v: 1 if v > 0 else -1
    off_x, off_y, off_z = sign(dx), sign(dy) * nx, sign(dz)
    state = dict(offset=int(y0) * nx + int(x0), z_mask=((1 << 16) | 1) << int(z0))
    dist = np.sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1) + (z0 - z1) * (z0 - z1))
    with np.errstate(all="ignore"):
        scale = _min(f64(1.0), f64(max_length) / dist)

    def grid_off(d):
        state["offset"] += d

    def z_off(d):
        state["z_mask"] = (state["z_mask"] << 1) if d > 0 else (state["z_mask"] >> 1)

    def bresenham(off_a, off_b, off_c, abs_da, abs_db, abs_dc, error_b, error_c, offset_a, offset_b, offset_c, length):
        for _ in range(min(length, abs_da)):
            cols[state["offset"]] &= np.uint32(~state["z_mask"] & 0xFFFFFFFF)
            off_a(offset_a)
            error_b += abs_db
            error_c += abs_dc
            if error_b >= abs_da:
                off_b(offset_b)
                error_b -= abs_da
            if error_c >= abs_da:
                off_c(offset_c)
                error_c -= abs_da
        cols[state["offset"]] &= np.uint32(~state["z_mask"] & 0xFFFFFFFF)

    if abs_dx >= max(abs_dy, abs_dz):
        bresenham(grid_off, grid_off, z_off, abs_dx, abs_dy, abs_dz, abs_dx // 2, abs_dx // 2, off_x, off_y, off_z, int(scale * abs_dx))
    elif abs_dy >= abs_dz:
        bresenham(grid_off, grid_off, z_off, abs_dy, abs_dx, abs_dz, abs_dy // 2, abs_dy // 2, off_y, off_x, off_z, int(scale * abs_dy))
    else:
        bresenham(z_off, grid_off, grid_off, abs_dz, abs_dx, abs_dy, abs_dz // 2, abs_dz // 2, off_z, off_x, off_y, int(scale * abs_dz))


# ------------------------------------------------------------------------------------------------ the endpoint scenario
# 60 x 60 cells of 0.05 m, origin_z 0, z_resolution 0.2, 10 voxels, max_obstacle_height 1.5; two robots with their own origins
END_NX = END_NY = 60
END_RES, END_ORIGIN_Z, END_Z_RES, END_Z_VOXELS, END_MAX_H = 0.05, 0.0, 0.2, 10, 1.5
END_ORIGINS = [(-1.0, 0.5), (0.25, -0.75)]
MARGIN = 1e-9  # cells


def end_geometry(robot):
    ox, oy = END_ORIGINS[robot]
    return Geometry(ox, oy, END_RES, END_NX, END_NY, END_ORIGIN_Z, END_Z_RES, END_Z_VOXELS, END_MAX_H)


def end_cloud(robot, n=130, seed=0):
    """n points around a sensor inside the map: the first 16 are placed by hand - 2 above max_obstacle_height, 2 below the
    floor, 2 beyond each of the four map edges, 4 nearer than 2 * res to the sensor (scaling_fact 0) - the rest are drawn from
    a box that overhangs the map by 0.8 m on every side and in z.  Returns (points float32 (n, 3), sensor origin)."""
    ox, oy = END_ORIGINS[robot]
    sensor = (ox + 1.37 + 0.11 * robot, oy + 1.62 - 0.07 * robot, 0.93)
    sx, sy, sz = sensor
    hand = [
        (sx + 0.6, sy + 0.3, 1.9), (sx - 0.4, sy + 0.7, 2.2),            # above max_obstacle_height
        (sx + 0.8, sy - 0.5, -0.3), (sx - 0.7, sy - 0.2, -0.15),          # below the floor
        (ox - 0.5, sy + 0.21, 0.6), (ox - 0.2, sy - 0.43, 1.1),           # beyond x = origin_x
        (ox + 3.4, sy + 0.33, 0.7), (ox + 3.9, sy - 0.61, 0.4),           # beyond map_end_x
        (sx + 0.17, oy - 0.6, 0.5), (sx - 0.29, oy - 0.1, 1.2),           # beyond y = origin_y
        (sx + 0.23, oy + 3.3, 0.8), (sx - 0.31, oy + 3.7, 0.3),           # beyond map_end_y
        (sx + 0.03, sy + 0.02, sz + 0.01), (sx - 0.05, sy, sz), (sx, sy - 0.06, sz - 0.04), (sx + 0.01, sy + 0.01, sz + 0.08),
    ]
    rs = np.random.RandomState(100 * seed + robot)
    rest = np.stack([rs.uniform(ox - 0.8, ox + 3.8, n - len(hand)), rs.uniform(oy - 0.8, oy + 3.8, n - len(hand)),
                     rs.uniform(-0.4, 2.3, n - len(hand))], axis=1)
    return np.concatenate([np.array(hand), rest]).astype(np.float32)[:n], sensor


def end_observations(robot):
    """the three observations of a robot, as Fleet.stage_observations takes them (without the instance)"""
    pts, sensor = end_cloud(robot)
    ox, oy = END_ORIGINS[robot]
    rs = np.random.RandomState(7 + robot)
    mark = np.stack([rs.uniform(ox + 0.2, ox + 2.8, 40), rs.uniform(oy + 0.2, oy + 2.8, 40), rs.uniform(0.1, 1.4, 40)], axis=1).astype(np.float32)
    off = np.stack([rs.uniform(ox + 0.2, ox + 2.8, 20), rs.uniform(oy + 0.2, oy + 2.8, 20), rs.uniform(0.1, 1.4, 20)], axis=1).astype(np.float32)
    return [dict(points=pts, origin=sensor, obstacle_range=2.5, raytrace_range=3.0, marking=True, clearing=True),
            dict(points=mark, origin=sensor, obstacle_range=2.5, raytrace_range=3.0, marking=True, clearing=False),
            dict(points=off, origin=(ox - 0.4, oy + 1.0, 0.9), obstacle_range=2.5, raytrace_range=3.0, marking=False, clearing=True)]


def assert_decisions_have_margin(result):
    """No point's kept / dropped decision in the final worldToMap3DFloat may rest on less than MARGIN cells - except where the
    reference's own clip puts the coordinate ONTO the threshold it is then compared with (a ray cut at x = origin_x, y =
    origin_y or z = origin_z: wpx = ox + a * ((origin_x - ox) / a) is origin_x up to the rounding of that very expression,
    so which side it lands on is decided by IEEE rounding in the reference itself).  Those rays are part of what the endpoint
    cloud shows - the issue's cases name them - and the device runs the same fp64 sequence unfused, so they stay in and are
    counted; every other point must keep the margin."""
    free = ~result["on_threshold"]
    assert (result["margin"][free] > MARGIN).all(), "a kept / dropped decision rests on less than 1e-9 cell: choose another seed"
    return int(result["on_threshold"].sum())
