"""numpy restatement of costmap_3d's layered map update as include/navgpu_costmap3d_layers.h states it: PointCloudLayer3D,
Static2DLayer3D, CylinderClearingLayer3D, LayeredCostmap3D::updateMap and Costmap3DTo2DLayer on dense state volumes.

A volume is a uint8 array [x, y, z] of cell states - 0 absent (the reference's missing node), 1 FREE, 2 NONLETHAL, 3 LETHAL - so
that "the higher class" is the larger number and nothing here is a bit trick: the kernels work on one-hot bit planes, this file
on one byte per cell with plain comparisons.  Octomap, PCL and tf are not at hand: this is a restatement of the rules, written
from them, and the closed forms in tests/test_costmap3d_layers_reference.py hold it in place."""
import numpy as np

ABSENT, FREE, NONLETHAL, LETHAL = 0, 1, 2, 3
POINT_CLOUD, STATIC_2D, CYLINDER_CLEARING = 0, 1, 2
OVERWRITE, MAXIMUM, IF_UNKNOWN, NOTHING = 0, 1, 2, 99
EMPTY_BOUNDS = (1e6, 1e6, -1e6, -1e6)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def origin_keys(origin, res):
    """llround(origin / resolution) per axis; the origin must be a multiple of the resolution to 1e-6 of a cell"""
    f = np.asarray(origin, np.float64) / res
    assert np.all(np.abs(f - np.rint(f)) <= 1e-6), "origin is not aligned"
    return np.rint(f).astype(np.int64)


def coord_to_cell(c, res, ok):
    """octomap's coordToKey less the origin's key: floor(c * (1 / res)) - ok; (cells int64, finite bool)"""
    c = np.asarray(c, np.float64)
    finite = np.isfinite(c)
    f = np.floor(np.where(finite, c, 0.0) * (1.0 / res))
    finite = finite & (np.abs(f) < 4.0e18)  # (beyond any key: off the extents)
    return np.where(finite, f, 0.0).astype(np.int64) - ok, finite


def cell_centre(i, ok, res):
    """keyToCoord"""
    return (np.asarray(ok + i, np.float64) + 0.5) * res


def transform_points(xyz, tf):
    """r0*x + r1*y + r2*z + t in fp64, left to right, stored as float (pcl::transformPointCloud)"""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    t = [np.float64(v) for v in tf]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([t[0] * x + t[1] * y + t[2] * z + t[9], t[3] * x + t[4] * y + t[5] * z + t[10], t[6] * x + t[7] * y + t[8] * z + t[11]], axis=1)
        return out.astype(np.float32)


def intensity_cost(intensity, free_intensity, lethal_intensity):
    """pointIntensityToCost in float, as written: the Cost (LETHAL 10, FREE -10, in between interpolated)"""
    i, f, l = np.float32(intensity), np.float32(free_intensity), np.float32(lethal_intensity)
    if i >= l:
        return np.float32(10.0)
    if i <= f:
        return np.float32(-10.0)
    with np.errstate(all="ignore"):
        return np.float32(np.float32(np.float32(i - f) / np.float32(l - f)) * np.float32(np.float32(10.0) - np.float32(-10.0))) + np.float32(-10.0)


def cost_class(cost):
    return LETHAL if cost >= np.float32(10.0) else FREE if cost <= np.float32(-10.0) else NONLETHAL


def cloud_cells(points, size, origin, res, tf=IDENTITY, has_intensity=False, free_intensity=0.0, lethal_intensity=1.0):
    """the cells of one cloud: (volume, number of points dropped).  Per cell the highest class wins."""
    points = np.asarray(points, np.float32).reshape(-1, 4 if has_intensity else 3)
    vol = np.zeros(size, np.uint8)
    ok = origin_keys(origin, res)
    world = transform_points(points[:, :3], tf)
    cells, finite = coord_to_cell(world, res, ok)
    clipped = 0
    for k in range(len(points)):
        c = cells[k]
        if not finite[k].all() or np.any(c < 0) or np.any(c >= np.asarray(size)):
            clipped += 1
            continue
        cls = cost_class(intensity_cost(points[k, 3], free_intensity, lethal_intensity)) if has_intensity else LETHAL
        vol[c[0], c[1], c[2]] = max(vol[c[0], c[1], c[2]], cls)
    return vol, clipped


def static_cells(grid, grid_origin_x, grid_origin_y, size, origin, res, height, lethal_cost_threshold=100, unknown_to_lethal=False):
    """Static2DLayer3D: each grid cell's centre at the level of `height`; (volume, number of cells dropped)"""
    grid = np.asarray(grid, np.int8)
    vol = np.zeros(size, np.uint8)
    ok = origin_keys(origin, res)
    kz, _ = coord_to_cell(height, res, ok[2])
    clipped = 0
    for j in range(grid.shape[0]):
        y = grid_origin_y + j * res + res / 2.0
        ky, _ = coord_to_cell(y, res, ok[1])
        for i in range(grid.shape[1]):
            x = grid_origin_x + i * res + res / 2.0
            kx, _ = coord_to_cell(x, res, ok[0])
            v = int(grid[j, i])
            if v < 0:
                if not unknown_to_lethal:
                    continue  # UNKNOWN: no cell
                cls = LETHAL
            else:
                cls = LETHAL if v >= lethal_cost_threshold else FREE
            if not (0 <= kx < size[0] and 0 <= ky < size[1] and 0 <= kz < size[2]):
                clipped += 1
                continue
            vol[kx, ky, kz] = cls
    return vol, clipped


def cylinder_columns(pose_xy, radius, size, origin, res):
    """the clearing set: columns in the clamped key box of pose +- radius whose centre satisfies x*x + y*y <= r*r; bool [x, y]"""
    ok = origin_keys(origin, res)
    cols = np.zeros(size[:2], bool)
    box = []
    for a in range(2):
        lo, _ = coord_to_cell(pose_xy[a] - radius, res, ok[a])
        hi, _ = coord_to_cell(pose_xy[a] + radius, res, ok[a])
        box.append((int(np.clip(lo, 0, size[a] - 1)), int(np.clip(hi, 0, size[a] - 1))))
    for ix in range(box[0][0], box[0][1] + 1):
        for iy in range(box[1][0], box[1][1] + 1):
            x = cell_centre(ix, ok[0], res) - pose_xy[0]
            y = cell_centre(iy, ok[1], res) - pose_xy[1]
            if x * x + y * y <= radius * radius:
                cols[ix, iy] = True
    return cols


def project_column(column, nonlethal_cost_2d=127):
    """the 2-D byte of one master column"""
    if np.any(column == LETHAL):
        return 254
    if np.any(column == NONLETHAL):
        return nonlethal_cost_2d
    if np.any(column == FREE):
        return 0
    return 255


def update_with_max(master, layer):
    """CostmapLayer::updateWithMax on single bytes"""
    if layer == 255:
        return master
    return layer if (master == 255 or master < layer) else master


def update_with_overwrite(master, layer):
    return master if layer == 255 else layer


def update_costs(master_grid, layer_grid, box, use_maximum):
    """over the cell box [min_i, max_i) x [min_j, max_j); grids are [y, x]"""
    out = master_grid.copy()
    rule = update_with_max if use_maximum else update_with_overwrite
    for j in range(box[1], box[3]):
        for i in range(box[0], box[2]):
            out[j, i] = rule(int(master_grid[j, i]), int(layer_grid[j, i]))
    return out


class LayeredMap:
    """one instance: a stack of layers (dicts: kind, enabled, combination_method and the kind's parameters), the master volume and the
    2-D layer [y, x]"""

    def __init__(self, size, origin, res, layers, nonlethal_cost_2d=127):
        self.size, self.origin, self.res = tuple(size), np.asarray(origin, np.float64), res
        self.layers = [dict(enabled=1, combination_method=MAXIMUM, **{k: v for k, v in l.items() if k not in ("enabled", "combination_method")}) for l in layers]
        for mine, given in zip(self.layers, layers):
            mine.update({k: given[k] for k in ("enabled", "combination_method") if k in given})
        self.nonlethal_cost_2d = nonlethal_cost_2d
        self.master = np.zeros(self.size, np.uint8)
        self.vol = [np.zeros(self.size, np.uint8) if l["kind"] != CYLINDER_CLEARING else None for l in self.layers]
        self.changed = [np.zeros(self.size, bool) if l["kind"] != CYLINDER_CLEARING else None for l in self.layers]
        self.prev = [None] * len(self.layers)
        self.full = True
        self.layer2d = np.full((self.size[1], self.size[0]), 255, np.uint8)

    def _replace(self, layer, new):
        self.changed[layer] |= self.vol[layer] != new
        self.vol[layer] = new

    def buffer_cloud(self, layer, points, tf=IDENTITY):
        l = self.layers[layer]
        assert l["kind"] == POINT_CLOUD
        new, clipped = cloud_cells(points, self.size, self.origin, self.res, tf, bool(l.get("cloud_has_intensity", 0)), l.get("free_intensity", 0.0),
                                   l.get("lethal_intensity", 1.0))
        self._replace(layer, new)
        return clipped

    def set_static_grid(self, layer, grid, grid_origin_x, grid_origin_y):
        l = self.layers[layer]
        assert l["kind"] == STATIC_2D
        new, clipped = static_cells(grid, grid_origin_x, grid_origin_y, self.size, self.origin, self.res, l.get("height", 0.0),
                                    l.get("lethal_cost_threshold", 100), bool(l.get("unknown_to_lethal", 0)))
        self._replace(layer, new)
        return clipped

    def layer_set(self, layer, enabled, combination_method):
        l = self.layers[layer]
        if (bool(l["enabled"]) != bool(enabled) or l["combination_method"] != combination_method) and l["kind"] != CYLINDER_CLEARING:
            self.changed[layer] |= self.vol[layer] != ABSENT
        l["enabled"], l["combination_method"] = enabled, combination_method

    def reset(self):
        self.master[:] = 0
        for k, l in enumerate(self.layers):
            if l["kind"] == CYLINDER_CLEARING:
                self.prev[k] = None
            else:
                self.vol[k][:] = 0
                self.changed[k][:] = False
        self.full = True

    def update(self, pose_xyz):
        """LayeredCostmap3D::updateMap, non-rolling, with the projection; returns the 2-D bounds"""
        bounds = np.zeros(self.size, bool)
        current = [None] * len(self.layers)
        for k, l in enumerate(self.layers):  # updateBounds
            if l["kind"] == CYLINDER_CLEARING:
                if self.prev[k] is not None:
                    bounds |= self.prev[k][:, :, None]
                if l["enabled"]:
                    current[k] = cylinder_columns(pose_xyz[:2], abs(l["radius"]), self.size, self.origin, self.res)
                    bounds |= current[k][:, :, None]
                self.prev[k] = current[k]
            else:
                bounds |= self.changed[k]
                self.changed[k] = np.zeros(self.size, bool)
        if self.full:
            bounds[:] = True
            self.full = False
        self.master[bounds] = ABSENT
        for k, l in enumerate(self.layers):  # updateCosts, in order
            if not l["enabled"]:
                continue
            if l["kind"] == CYLINDER_CLEARING:
                self.master[current[k]] = ABSENT
                continue
            v, m = self.vol[k], l["combination_method"]
            present = bounds & (v != ABSENT)
            if m == OVERWRITE:
                take = present
            elif m == MAXIMUM:
                take = present & (v > self.master)
            elif m == IF_UNKNOWN:
                take = present & (self.master == ABSENT)
            else:
                take = np.zeros(self.size, bool)
            self.master[take] = v[take]
        columns = bounds.any(axis=2)  # [x, y]
        xs, ys = np.nonzero(columns)
        for x, y in zip(xs, ys):
            self.layer2d[y, x] = project_column(self.master[x, y], self.nonlethal_cost_2d)
        if not len(xs):
            return EMPTY_BOUNDS
        return (self.origin[0] + xs.min() * self.res, self.origin[1] + ys.min() * self.res, self.origin[0] + (xs.max() + 1) * self.res,
                self.origin[1] + (ys.max() + 1) * self.res)


def to_words(vol, state):
    """the bit plane of one state as the device holds it: (size_y, size_x) uint64, bit z"""
    sx, sy, sz = vol.shape
    out = np.zeros((sy, sx), np.uint64)
    for z in range(sz):
        out |= (vol[:, :, z].T == state).astype(np.uint64) << np.uint64(z)
    return out


def bool_words(mask):
    sx, sy, sz = mask.shape
    out = np.zeros((sy, sx), np.uint64)
    for z in range(sz):
        out |= mask[:, :, z].T.astype(np.uint64) << np.uint64(z)
    return out
