"""Costmap3D: thin Python handle over navgpu_costmap3d_* - costmap_3d::Costmap3DQuery for batches of poses on one GPU.

  set_origin / origin     the frame of an instance's grid
  set_boxes               Costmap3DQuery::updateCostmap and an octomap update's deltas   (costmap_3d/src/costmap_3d_query.cpp:128-287)
  set_mesh                Costmap3DQuery::updateMeshResource with padPoints              (:413-449; costmap_3d_query.h:332-350)
  query                   Costmap3DROS::processPlanCost3D over footprintCollision / footprintCost / footprintDistance
                          (costmap_3d/src/costmap_3d_ros.cpp:464-616; costmap_3d_query.cpp:493-521, 586-970)
  footprint_costs         base_local_planner::Costmap3DModel::footprintCost              (base_local_planner/src/costmap_3d_model.cpp:61-79)
  columns / set_columns   the resident bit volumes themselves
  configure_layers, layer_set, buffer_clouds, set_static_grid, update, reset, layer2d, update_costs_2d, layer_columns, free_columns
                          the layered map update from point clouds and its projection into 2-D (include/navgpu_costmap3d_layers.h):
                          PointCloudLayer3D, Static2DLayer3D, CylinderClearingLayer3D, LayeredCostmap3D::updateMap, Costmap3DTo2DLayer
  roll, reset_bounding_box
                          rolling windows and Costmap3DROS::resetBoundingBox (include/navgpu_costmap3d_rolling.h):
                          LayeredCostmap3D::updateMap's rolling part, CostmapLayer3D::resetBoundingBox
  configure_publisher, export, update_cells, resubscribe
                          the maps' way out of a handle and into a layer as pruned octree leaves (include/navgpu_costmap3d_publish.h):
                          Costmap3DPublisher, CostmapLayer3D::updateCells, OctomapServerLayer3D's subscription
  leaves_to_boxes, boxes_to_leaves
                          leaves as set_boxes takes them, and back
  load_stl                a binary STL as (vertices, triangles), equal corners merged
  load_octomap_bt         an octomap binary tree (.bt) as its occupied leaves: centres, sizes, classes
All compute happens in libnavgpu.so on the GPU; this file only marshals numpy buffers and reads the two file formats.
"""
import ctypes as C
import struct

import numpy as np

from ._lib import (C3D_CELLS_BINARY, C3D_DISTANCE, C3D_EXPORT_FULL, C3D_LETHAL, C3D_REPLACE, C3D_ROLL_CENTRE, C3D_ROLL_ORIGIN, GRID_MASTER, C3dBox, C3dCloud, C3dLayer,
                   C3dLeaf, C3dRun, C3dRunResult, C3dUpdateMsg, Costmap3DDesc, check, lib)

BOX_DTYPE = np.dtype([("cx", "<f8"), ("cy", "<f8"), ("cz", "<f8"), ("size", "<f8"), ("cls", "<i4"), ("reserved", "<i4")])
RUN_DTYPE = np.dtype([("instance", "<u4"), ("first_pose", "<u4"), ("n_poses", "<u4")])
RUN_RESULT_DTYPE = np.dtype([("cost", "<f8"), ("n_lethal", "<i4"), ("first_lethal", "<i4"), ("n_done", "<i4"), ("reserved", "<i4")])
CLOUD_DTYPE = np.dtype([("instance", "<u4"), ("layer", "<u4"), ("first_point", "<u4"), ("n_points", "<u4"), ("transform", "<f8", 12)])
IDENTITY_TRANSFORM = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
assert CLOUD_DTYPE.itemsize == C.sizeof(C3dCloud)
assert BOX_DTYPE.itemsize == C.sizeof(C3dBox) and RUN_DTYPE.itemsize == C.sizeof(C3dRun) and RUN_RESULT_DTYPE.itemsize == C.sizeof(C3dRunResult)
LEAF_DTYPE = np.dtype([("key", "<i4", 3), ("level", "<u2"), ("cls", "<u2")])
UPDATE_MSG_DTYPE = np.dtype([("instance", "<u4"), ("update_seq", "<u4"), ("bounds_seq", "<u4"), ("universe", "<i4"), ("plain_map", "<i4"), ("first_value", "<u4"),
                             ("n_values", "<u4"), ("first_bound", "<u4"), ("n_bounds", "<u4"), ("n_forgotten", "<u4"), ("forgotten", "<i4", (2, 6))])
assert LEAF_DTYPE.itemsize == C.sizeof(C3dLeaf) == 16 and UPDATE_MSG_DTYPE.itemsize == C.sizeof(C3dUpdateMsg) == 88
NAVGPU_ERR_CAPACITY = -4
DBL_MAX = float(np.finfo(np.float64).max)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load_stl(path):
    """A binary STL -> (vertices (nv, 3) float64, triangles (nt, 3) uint32).  Corners with equal coordinates become one vertex,
    in order of first appearance; the facet normals are not used (the corner order gives the orientation)."""
    data = open(path, "rb").read()
    (nt,) = struct.unpack_from("<I", data, 80)
    if len(data) != 84 + 50 * nt:
        raise ValueError(f"{path}: not a binary STL ({len(data)} bytes for {nt} triangles)")
    rec = np.frombuffer(data, np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), count=nt, offset=84)
    index, vertices, triangles = {}, [], np.zeros((nt, 3), np.uint32)
    for t in range(nt):
        for k in range(3):
            key = rec["v"][t, k].tobytes()
            if key not in index:
                index[key] = len(vertices)
                vertices.append(rec["v"][t, k].astype(np.float64))
            triangles[t, k] = index[key]
    return np.array(vertices, np.float64).reshape(-1, 3), triangles


def read_octomap_bt(path):
    """An octomap binary tree file, whole: dict(res, depth, size, n_nodes, centres, sizes, classes, depths) of its occupied leaves.
    The text header ends at the `data` line (`depth N` is this fork's line; 16 without it).  Then, depth first, 2 bytes per inner
    node: child i is the bit pair (2j, 2j + 1) of byte i // 4, j = i & 3, least significant first - (0, 0) absent, (1, 0) free leaf,
    (0, 1) occupied leaf, (1, 1) inner node, whose record follows in child order.  Child i adds bit 0 of i to the x key, bit 1 to
    y, bit 2 to z; a leaf at depth d with key k has edge res * 2^(N - d) and centre (k + 0.5) * edge - 2^(N - 1) * res."""
    data = open(path, "rb").read()
    at = data.index(b"\ndata\n") + 6
    header = {}
    for line in data[:at].decode("ascii", "replace").splitlines():
        parts = line.split()
        if len(parts) == 2 and not line.startswith("#"):
            header[parts[0]] = parts[1]
    res, depth, size = float(header["res"]), int(header.get("depth", 16)), int(header["size"])
    payload = data[at:]
    pos, n_nodes = 0, 1
    centres, sizes, depths = [], [], []
    stack = [(0, 0, 0, 0)]  # inner nodes whose record is next, last on top: (depth, kx, ky, kz)
    while stack:
        d, kx, ky, kz = stack.pop()
        if pos + 2 > len(payload):
            raise ValueError(f"{path}: the tree ends before its payload does")
        b = payload[pos:pos + 2]
        pos += 2
        inner = []
        for i in range(8):
            pair = (b[i // 4] >> (2 * (i & 3))) & 3  # bit 2j is the pair's first
            if pair == 0:
                continue
            n_nodes += 1
            cx, cy, cz = 2 * kx + (i & 1), 2 * ky + ((i >> 1) & 1), 2 * kz + ((i >> 2) & 1)
            if pair == 3:
                inner.append((d + 1, cx, cy, cz))
            elif pair == 2:  # (0, 1): occupied
                edge = res * 2.0 ** (depth - d - 1)
                centres.append([(k + 0.5) * edge - 2.0 ** (depth - 1) * res for k in (cx, cy, cz)])
                sizes.append(edge)
                depths.append(d + 1)
        stack.extend(reversed(inner))
    assert pos == len(payload), f"{path}: {len(payload) - pos} payload bytes left over"
    assert n_nodes == size, f"{path}: {n_nodes} nodes read, the header says {size}"
    return dict(res=res, depth=depth, size=size, n_nodes=n_nodes, centres=np.array(centres, np.float64).reshape(-1, 3),
                sizes=np.array(sizes, np.float64), classes=np.full(len(sizes), C3D_LETHAL, np.int32), depths=np.array(depths, np.int32))


def load_octomap_bt(path):
    """the occupied leaves of a .bt file as set_boxes takes them: (centres (n, 3), sizes (n,), classes (n,))"""
    t = read_octomap_bt(path)
    return t["centres"], t["sizes"], t["classes"]


def leaves_to_boxes(leaves, resolution):
    """leaves (LEAF_DTYPE) -> (centres (n, 3), sizes (n,), classes (n,)) as set_boxes takes them (which knows LETHAL and NONLETHAL only)"""
    l = np.asarray(leaves, LEAF_DTYPE).reshape(-1)
    edge = np.ldexp(float(resolution), l["level"].astype(np.int32))
    return l["key"].astype(np.float64) * float(resolution) + 0.5 * edge[:, None], edge, l["cls"].astype(np.int32)


def boxes_to_leaves(centres, sizes, classes, resolution):
    """the inverse of leaves_to_boxes: boxes whose size is resolution * 2^k and whose lower corner lies on the lattice"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    size = np.broadcast_to(np.asarray(sizes, np.float64), (len(c),))
    level = np.rint(np.log2(size / float(resolution))).astype(np.int64)
    key = (c - 0.5 * size[:, None]) / float(resolution)
    assert np.all(np.abs(size - np.ldexp(float(resolution), level.astype(np.int32))) <= 1e-9) and np.all(np.abs(key - np.rint(key)) <= 1e-6), "not leaves of the lattice"
    out = np.zeros(len(c), LEAF_DTYPE)
    out["key"], out["level"], out["cls"] = np.rint(key), level, np.broadcast_to(np.asarray(classes), (len(c),))
    return out


class Costmap3D:
    def __init__(self, n_instances, size_x, size_y, size_z, resolution, max_triangles=64, max_boxes=1 << 16, max_poses=1 << 12, device=0):
        self.L = lib()
        self.n, self.size_x, self.size_y, self.size_z, self.resolution = n_instances, size_x, size_y, size_z, float(resolution)
        desc = Costmap3DDesc(n_instances, size_x, size_y, size_z, resolution, max_triangles, max_boxes, max_poses, device)
        h = C.c_void_p()
        check(self.L.navgpu_costmap3d_create(C.byref(desc), C.byref(h)), "navgpu_costmap3d_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.navgpu_costmap3d_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_origin(self, instance, origin_xyz):
        o = np.ascontiguousarray(origin_xyz, np.float64).reshape(3)
        check(self.L.navgpu_costmap3d_set_origin(self.h, instance, _ptr(o)), "navgpu_costmap3d_set_origin")

    def origin(self, instance):
        o = np.zeros(3)
        check(self.L.navgpu_costmap3d_get_origin(self.h, instance, _ptr(o)), "navgpu_costmap3d_get_origin")
        return o

    def set_boxes(self, instance, centres, sizes, classes=None, mode=C3D_REPLACE):
        """centres (n, 3), sizes (n,) or one size, classes (n,) or None (LETHAL).  Returns the number of cells that fell outside the extents."""
        c = np.asarray(centres, np.float64).reshape(-1, 3)
        boxes = np.zeros(len(c), BOX_DTYPE)
        boxes["cx"], boxes["cy"], boxes["cz"] = c[:, 0], c[:, 1], c[:, 2]
        boxes["size"] = sizes
        boxes["cls"] = C3D_LETHAL if classes is None else classes
        clipped = C.c_uint32(0)
        check(self.L.navgpu_costmap3d_set_boxes(self.h, instance, mode, _ptr(boxes), len(boxes), C.byref(clipped)), "navgpu_costmap3d_set_boxes")
        return clipped.value

    def set_columns(self, instance, lethal=None, nonlethal=None):
        planes = [None if p is None else np.ascontiguousarray(p, np.uint64).reshape(self.size_y, self.size_x) for p in (lethal, nonlethal)]
        check(self.L.navgpu_costmap3d_columns_upload(self.h, instance, _ptr(planes[0]), _ptr(planes[1])), "navgpu_costmap3d_columns_upload")

    def columns(self, instance):
        """(lethal, nonlethal): (size_y, size_x) uint64 each, bit z of a word is cell (x, y, z)"""
        lethal, nonlethal = np.zeros((self.size_y, self.size_x), np.uint64), np.zeros((self.size_y, self.size_x), np.uint64)
        check(self.L.navgpu_costmap3d_columns_download(self.h, instance, _ptr(lethal), _ptr(nonlethal)), "navgpu_costmap3d_columns_download")
        return lethal, nonlethal

    def set_mesh(self, vertices, triangles, padding=0.0):
        """Returns whether the mesh is closed and consistently oriented (an open mesh is a surface: no interior test)."""
        v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        closed = C.c_int32(0)
        check(self.L.navgpu_costmap3d_set_mesh(self.h, _ptr(v), len(v), _ptr(t), len(t), float(padding), C.byref(closed)), "navgpu_costmap3d_set_mesh")
        return bool(closed.value)

    @staticmethod
    def _runs(runs, n_poses):
        if runs is None:
            runs = [(0, 0, n_poses)]
        r = np.zeros(len(runs), RUN_DTYPE)
        for k, (instance, first, count) in enumerate(runs):
            r[k] = (instance, first, count)
        return r

    def query(self, poses, runs=None, mode=C3D_DISTANCE, regions=None, obstacles=None, region_scale=(0.0, 0.0, 0.0), distance_limit=DBL_MAX,
              lazy=False, pose_costs=None):
        """poses (n, 7) {x, y, z, qx, qy, qz, qw}; runs a list of (instance, first_pose, n_poses), default one run of every pose on
        instance 0.  Returns (pose_costs (n,), results: RUN_RESULT_DTYPE per run).  pose_costs, when given, is written in place:
        with lazy the entries behind a run's first lethal pose keep what they held (NaN in a fresh array)."""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        r = self._runs(runs, len(p))
        reg = None if regions is None else np.ascontiguousarray(regions, np.uint8)
        obs = None if obstacles is None else np.ascontiguousarray(obstacles, np.uint8)
        assert all(a is None or len(a) == len(p) for a in (reg, obs))
        scale = np.ascontiguousarray(region_scale, np.float64).reshape(3)
        costs = np.full(len(p), np.nan) if pose_costs is None else pose_costs
        assert costs.dtype == np.float64 and costs.flags.c_contiguous and len(costs) == len(p)
        results = np.zeros(len(r), RUN_RESULT_DTYPE)
        check(self.L.navgpu_costmap3d_query(self.h, len(r), _ptr(r), _ptr(p), mode, _ptr(reg), _ptr(obs), _ptr(scale), float(distance_limit), int(lazy),
                                            _ptr(costs), _ptr(results)), "navgpu_costmap3d_query")
        return costs, results

    def footprint_costs(self, poses_xyth, runs=None):
        """poses (n, 3) {x, y, theta}.  Returns (costs (n,), first_illegal per run)."""
        p = np.ascontiguousarray(poses_xyth, np.float64).reshape(-1, 3)
        r = self._runs(runs, len(p))
        costs, first = np.full(len(p), np.nan), np.zeros(len(r), np.int32)
        check(self.L.navgpu_costmap3d_footprint_costs(self.h, len(r), _ptr(r), _ptr(p), _ptr(costs), _ptr(first)), "navgpu_costmap3d_footprint_costs")
        return costs, first

    # ---- the layered map update (include/navgpu_costmap3d_layers.h) ----
    def configure_layers(self, layers, nonlethal_cost_2d=127):
        """layers: dicts with the fields of navgpu_c3d_layer (kind and whatever its kind reads; enabled defaults to 1, the method to
        Maximum, max_cloud_points to 65536), in the order the stack applies them."""
        recs = (C3dLayer * len(layers))()
        for k, spec in enumerate(layers):
            d = dict(enabled=1, combination_method=1, max_cloud_points=1 << 16)
            d.update(spec)
            recs[k] = C3dLayer(**d)
        check(self.L.navgpu_costmap3d_configure_layers(self.h, recs, len(layers), int(nonlethal_cost_2d)), "navgpu_costmap3d_configure_layers")

    def layer_set(self, layer, enabled, combination_method):
        check(self.L.navgpu_costmap3d_layer_set(self.h, layer, int(enabled), int(combination_method)), "navgpu_costmap3d_layer_set")

    def buffer_clouds(self, clouds, points):
        """clouds: a list of (instance, layer, first_point, n_points[, transform12]); points (n, 3) or (n, 4) float32 by the layers'
        format.  Returns the number of points dropped per cloud."""
        c = np.zeros(len(clouds), CLOUD_DTYPE)
        for k, rec in enumerate(clouds):
            c[k] = tuple(rec[:4]) + (tuple(rec[4]) if len(rec) > 4 else IDENTITY_TRANSFORM,)
        p = np.ascontiguousarray(points, np.float32)
        assert p.ndim == 2 and p.shape[1] in (3, 4)
        clipped = np.zeros(len(c), np.uint32)
        check(self.L.navgpu_costmap3d_buffer_clouds(self.h, _ptr(c), len(c), _ptr(p), len(p), _ptr(clipped)), "navgpu_costmap3d_buffer_clouds")
        return clipped

    def set_static_grid(self, instance, layer, occupancy, origin_x, origin_y):
        """occupancy (height, width) int8 at the map's resolution.  Returns the number of cells that fell outside the extents."""
        g = np.ascontiguousarray(occupancy, np.int8)
        assert g.ndim == 2
        clipped = C.c_uint32(0)
        check(self.L.navgpu_costmap3d_set_static_grid(self.h, instance, layer, _ptr(g), g.shape[1], g.shape[0], float(origin_x), float(origin_y),
                                                      C.byref(clipped)), "navgpu_costmap3d_set_static_grid")
        return clipped.value

    def update(self, instances, robot_poses_xyz):
        """Returns the 2-D bounds (n, 4) = min_x, min_y, max_x, max_y per listed instance ((1e6, 1e6, -1e6, -1e6): none)."""
        ins = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        poses = np.ascontiguousarray(robot_poses_xyz, np.float64).reshape(-1, 3)
        assert len(poses) == len(ins)
        bounds = np.zeros((len(ins), 4))
        check(self.L.navgpu_costmap3d_update(self.h, len(ins), _ptr(ins), _ptr(poses), _ptr(bounds)), "navgpu_costmap3d_update")
        return bounds

    def reset(self, instances=None):
        ins = np.arange(self.n, dtype=np.uint32) if instances is None else np.ascontiguousarray(instances, np.uint32).reshape(-1)
        check(self.L.navgpu_costmap3d_reset(self.h, len(ins), _ptr(ins)), "navgpu_costmap3d_reset")

    def layer2d(self, instance, x0=0, y0=0, xn=None, yn=None):
        xn = self.size_x if xn is None else xn
        yn = self.size_y if yn is None else yn
        out = np.zeros((max(yn - y0, 0), max(xn - x0, 0)), np.uint8)
        check(self.L.navgpu_costmap3d_layer2d_download(self.h, instance, x0, y0, xn, yn, _ptr(out)), "navgpu_costmap3d_layer2d_download")
        return out

    def update_costs_2d(self, fleet, instances, boxes_ij, use_maximum=True):
        """Costmap3DTo2DLayer::updateCosts into the fleet's master grid: boxes_ij (n, 4) = min_i, min_j, max_i, max_j.  The fleet
        must be idle meanwhile."""
        ins = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        boxes = np.ascontiguousarray(boxes_ij, np.int32).reshape(-1, 4)
        assert len(boxes) == len(ins)
        ptr, stride = fleet.grid_device(GRID_MASTER)
        check(self.L.navgpu_costmap3d_layer2d_update_costs(self.h, len(ins), _ptr(ins), ptr, stride, fleet.desc.n_instances, fleet.desc.size_x,
                                                           fleet.desc.size_y, _ptr(boxes), int(bool(use_maximum))),
              "navgpu_costmap3d_layer2d_update_costs")

    def layer_columns(self, instance, layer):
        """(lethal, nonlethal, free, changed) of a costmap layer: (size_y, size_x) uint64 each"""
        planes = [np.zeros((self.size_y, self.size_x), np.uint64) for _ in range(4)]
        check(self.L.navgpu_costmap3d_layer_columns_download(self.h, instance, layer, *[_ptr(p) for p in planes]), "navgpu_costmap3d_layer_columns_download")
        return tuple(planes)

    def free_columns(self, instance):
        free = np.zeros((self.size_y, self.size_x), np.uint64)
        check(self.L.navgpu_costmap3d_free_columns_download(self.h, instance, _ptr(free)), "navgpu_costmap3d_free_columns_download")
        return free

    # ---- rolling maps and resetBoundingBox (include/navgpu_costmap3d_rolling.h) ----
    def roll(self, instances, robot_xy=None, origin_xy=None):
        """Moves the listed instances' windows: round the robots' positions robot_xy (n, 2), or to the origins origin_xy (n, 2) - exactly
        one of the two.  Returns the shifts (n, 2) = dx, dy in cells.  A cycle is roll, then buffer_clouds, then update."""
        assert (robot_xy is None) != (origin_xy is None), "give robot_xy or origin_xy"
        ins = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        targets = np.ascontiguousarray(origin_xy if robot_xy is None else robot_xy, np.float64).reshape(-1, 2)
        assert len(targets) == len(ins)
        shifts = np.zeros((len(ins), 2), np.int32)
        check(self.L.navgpu_costmap3d_roll(self.h, len(ins), _ptr(ins), C3D_ROLL_ORIGIN if robot_xy is None else C3D_ROLL_CENTRE, _ptr(targets),
                                           _ptr(shifts)), "navgpu_costmap3d_roll")
        return shifts

    def reset_bounding_box(self, instances, boxes, layers):
        """boxes (n, 6) = min x, y, z, max x, y, z per listed instance; layers: the indices of the layers to clear inside them (only
        POINT_CLOUD layers hold anything the call deletes)."""
        ins = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
        assert len(b) == len(ins)
        mask = 0
        for l in layers:
            assert 0 <= int(l) < 32
            mask |= 1 << int(l)
        check(self.L.navgpu_costmap3d_reset_bounding_box(self.h, len(ins), _ptr(ins), _ptr(b), mask), "navgpu_costmap3d_reset_bounding_box")

    # ---- publishing: pruned octree leaves out of the handle and into a layer (include/navgpu_costmap3d_publish.h) ----
    def configure_publisher(self, enabled=True):
        check(self.L.navgpu_costmap3d_publisher_configure(self.h, int(bool(enabled))), "navgpu_costmap3d_publisher_configure")

    def export(self, instances, mode=C3D_EXPORT_FULL):
        """Returns (msgs: UPDATE_MSG_DTYPE per listed instance, values, bounds: LEAF_DTYPE arrays the messages' ranges index).  The
        arrays have the capacity of the last export; a call they are too small for commits nothing, says how many leaves there are
        and is repeated with room."""
        ins = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        msgs = np.zeros(len(ins), UPDATE_MSG_DTYPE)
        cap_v, cap_b = getattr(self, "_export_capacity", (0, 0))
        for _ in range(2):
            values, bounds = np.zeros(max(cap_v, 1), LEAF_DTYPE), np.zeros(max(cap_b, 1), LEAF_DTYPE)
            rc = self.L.navgpu_costmap3d_export(self.h, len(ins), _ptr(ins), int(mode), cap_v, _ptr(values), cap_b, _ptr(bounds), _ptr(msgs))
            if rc != NAVGPU_ERR_CAPACITY:
                break
            cap_v, cap_b = max(cap_v, int(msgs["n_values"].sum())), max(cap_b, int(msgs["n_bounds"].sum()))
        check(rc, "navgpu_costmap3d_export")
        self._export_capacity = (cap_v, cap_b)
        return msgs, values[:int(msgs["n_values"].sum())].copy(), bounds[:int(msgs["n_bounds"].sum())].copy()

    def export_counts(self, instances, mode=C3D_EXPORT_FULL):
        """the messages with their counts alone; nothing is committed"""
        ins = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        msgs = np.zeros(len(ins), UPDATE_MSG_DTYPE)
        check(self.L.navgpu_costmap3d_export(self.h, len(ins), _ptr(ins), int(mode), 0, None, 0, None, _ptr(msgs)), "navgpu_costmap3d_export")
        return msgs

    def update_cells(self, msgs, layers, values, bounds=None, cell_mode=C3D_CELLS_BINARY):
        """msgs (UPDATE_MSG_DTYPE; instance is the destination) into the layers layers[i]; returns the verdict per message."""
        m = np.ascontiguousarray(msgs, UPDATE_MSG_DTYPE).reshape(-1)
        lay = np.ascontiguousarray(layers, np.uint32).reshape(-1)
        assert len(lay) == len(m)
        v = np.ascontiguousarray(values, LEAF_DTYPE).reshape(-1)
        b = np.zeros(0, LEAF_DTYPE) if bounds is None else np.ascontiguousarray(bounds, LEAF_DTYPE).reshape(-1)
        verdicts = np.zeros(len(m), np.int32)
        check(self.L.navgpu_costmap3d_layer_update_cells(self.h, len(m), _ptr(m), _ptr(lay), int(cell_mode), _ptr(v) if len(v) else None, len(v),
                                                         _ptr(b) if len(b) else None, len(b), _ptr(verdicts)), "navgpu_costmap3d_layer_update_cells")
        return verdicts

    def resubscribe(self, instance, layer):
        check(self.L.navgpu_costmap3d_layer_resubscribe(self.h, instance, layer), "navgpu_costmap3d_layer_resubscribe")
