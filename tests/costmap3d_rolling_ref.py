"""numpy restatement of costmap_3d's rolling window and resetBoundingBox as include/navgpu_costmap3d_rolling.h states them, on top
of the layered yardstick (tests/costmap3d_layers_ref.py): LayeredCostmap3D::updateMap's rolling part, CostmapLayer3D::updateBounds'
deletion outside the rolled box, Costmap3DTo2DLayer's origin change and CostmapLayer3D::resetBoundingBox.

A map is a window of size_x x size_y columns at an integer key origin; a roll by (dx, dy) cells sends the column at (x, y) to
(x - dx, y - dy), what leaves is forgotten and what enters is absent.  The dense volumes are shifted with plain slicing: nothing
here is a bit trick.  The closed forms in tests/test_costmap3d_rolling_reference.py hold this file in place."""
import numpy as np

import costmap3d_layers_ref as ref


def shifted(a, dx, dy, empty):
    """out[x, y, ...] = a[x + dx, y + dy, ...] where that lies inside a, else `empty`; a is indexed [x, y, ...]"""
    out = np.full_like(a, empty)
    sx, sy = a.shape[0], a.shape[1]
    x_lo, x_hi = max(0, -dx), min(sx, sx - dx)  # the destination columns that have a source
    y_lo, y_hi = max(0, -dy), min(sy, sy - dy)
    if x_lo < x_hi and y_lo < y_hi:
        out[x_lo:x_hi, y_lo:y_hi] = a[x_lo + dx:x_hi + dx, y_lo + dy:y_hi + dy]
    return out


def centre_key(robot, size, res):
    """the window's first key along one axis for a robot coordinate: LayeredCostmap3D::updateMap with octomap::point3d's floats"""
    extent = np.float64(size) * np.float64(res)
    w = np.float64(np.float32(extent))
    half = w / np.float64(2.0)
    lower = np.float64(robot) - half
    m = np.float32(lower)
    factor = np.float64(1.0) / np.float64(res)
    scaled = np.float64(m) * factor
    return int(np.floor(scaled))


class RollingMap(ref.LayeredMap):
    """a LayeredMap whose window moves; `moved` is the mark the next update consumes"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.moved = False

    def _roll_to(self, keys):
        ok = ref.origin_keys(self.origin, self.res)
        dx, dy = int(keys[0] - ok[0]), int(keys[1] - ok[1])
        if dx == 0 and dy == 0:
            return (0, 0)
        self.master = shifted(self.master, dx, dy, ref.ABSENT)
        for k, l in enumerate(self.layers):
            if l["kind"] == ref.CYLINDER_CLEARING:
                continue  # (its previous set is a pose and a radius in world coordinates)
            self.vol[k] = shifted(self.vol[k], dx, dy, ref.ABSENT)
            self.changed[k] = shifted(self.changed[k], dx, dy, False)
        self.layer2d = shifted(self.layer2d.T, dx, dy, 255).T.copy()
        self.origin = np.array([keys[0] * self.res, keys[1] * self.res, self.origin[2]], np.float64)  # z does not roll
        self.moved = True
        return (dx, dy)

    def roll_centre(self, robot_xy):
        return self._roll_to([centre_key(robot_xy[a], self.size[a], self.res) for a in range(2)])

    def roll_origin(self, origin_xy):
        f = np.asarray(origin_xy, np.float64) / self.res
        assert np.all(np.abs(f - np.rint(f)) <= 1e-6), "the new origin is not aligned"
        return self._roll_to([int(v) for v in np.rint(f)])

    def reset(self):
        super().reset()
        self.moved = False

    def update(self, pose_xyz):
        bounds = super().update(pose_xyz)
        if not self.moved:
            return bounds
        self.moved = False
        return (self.origin[0], self.origin[1], self.origin[0] + self.size[0] * self.res, self.origin[1] + self.size[1] * self.res)

    def reset_bounding_box(self, box, layers):
        """box = (min x, y, z, max x, y, z); layers: indices.  Deletes the cells of the named POINT_CLOUD layers whose key lies between
        the corners' keys, both ends inclusive, inside the window; they become changed."""
        ok = ref.origin_keys(self.origin, self.res)
        lo, hi = [], []
        for a in range(3):
            if box[a] > box[3 + a]:
                return
            k0, _ = ref.coord_to_cell(box[a], self.res, ok[a])
            k1, _ = ref.coord_to_cell(box[3 + a], self.res, ok[a])
            lo.append(max(int(k0), 0))
            hi.append(min(int(k1), self.size[a] - 1))
            if lo[a] > hi[a]:
                return
        inside = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1), slice(lo[2], hi[2] + 1))
        for k in layers:
            if self.layers[k]["kind"] != ref.POINT_CLOUD:
                continue  # a STATIC_2D layer ignores the call; a cylinder layer keeps its set
            self.changed[k][inside] |= self.vol[k][inside] != ref.ABSENT
            self.vol[k][inside] = ref.ABSENT
