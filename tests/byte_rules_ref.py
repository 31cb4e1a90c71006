"""Restatements, written for the byte-table tests, of the reference's value rules that k_static_interpret, k_merge and
k_navfn_costmap replace - shared by tests/test_byte_rules_host.py (which pins them against the oracle on the CPU) and
tests/test_gpu_byte_rules.py (which compares the device against them).  Each one is a plain loop or a numpy mask written
from the reference text; Python's float is IEEE double, so int(v / L * 254.0) is the reference's own arithmetic.

  static_params / interpret_value / interpret   StaticLayer::onInitialize's clamp and wrap (costmap_2d/plugins/static_layer.cpp:75-81)
                                                and StaticLayer::interpretValue (:149-163) under incomingMap's loop (:199-207)
  reset_map                                     Costmap2D::resetMap (costmap_2d/src/costmap_2d.cpp:93-99) with the master's default
                                                (layered_costmap.cpp:53-56)
  update_with_max / _true_overwrite / _overwrite  CostmapLayer (costmap_2d/src/costmap_layer.cpp:62-86, 88-105, 107-124)
  static_update_costs                           StaticLayer::updateCosts (static_layer.cpp:287-337): non-rolling :295-298, the rolling
                                                branch's plain copy / std::max :329-332 for a static map in the master's geometry
  obstacle_update_costs                         ObstacleLayer::updateCosts' switch (plugins/obstacle_layer.cpp:437-447)
  update_map                                    LayeredCostmap::updateMap's reset -> static -> obstacle (layered_costmap.cpp:137-146)
  navfn_costarr                                 NavFn::setCostmap (navfn/src/navfn.cpp:227-287; constants navfn/include/navfn/navfn.h:49-67)
Nothing here reads the product."""
import functools

import numpy as np

NO_INFORMATION, LETHAL_OBSTACLE, INSCRIBED_INFLATED_OBSTACLE, FREE_SPACE = 255, 254, 253, 0  # cost_values.h:42-45


# --------------------------------------------------------------------------------------------------------- static layer
def static_params(lethal_cost_threshold, unknown_cost_value):
    """static_layer.cpp:80-81: lethal_threshold_ = max(min(temp, 100), 0); unknown_cost_value_ = temp, both unsigned char"""
    return max(min(int(lethal_cost_threshold), 100), 0), int(unknown_cost_value) & 0xFF


def interpret_value(value, track_unknown_space, trinary_costmap, lethal_threshold, unknown_cost_value):
    """static_layer.cpp:149-163, `value`, `lethal_threshold` and `unknown_cost_value` being unsigned chars"""
    if track_unknown_space and value == unknown_cost_value:
        return NO_INFORMATION
    elif not track_unknown_space and value == unknown_cost_value:
        return FREE_SPACE
    elif value >= lethal_threshold:
        return LETHAL_OBSTACLE
    elif trinary_costmap:
        return FREE_SPACE
    scale = float(value) / lethal_threshold  # double scale = (double) value / lethal_threshold_
    return int(scale * LETHAL_OBSTACLE) & 0xFF  # return scale * LETHAL_OBSTACLE: double -> unsigned char truncates


@functools.lru_cache(maxsize=None)
def interpret_table(track_unknown_space, trinary_costmap, lethal_cost_threshold, unknown_cost_value):
    """interpretValue of all 256 unsigned chars under the parameters AS CONFIGURED (before clamp and wrap)"""
    thr, unk = static_params(lethal_cost_threshold, unknown_cost_value)
    t = np.array([interpret_value(v, bool(track_unknown_space), bool(trinary_costmap), thr, unk) for v in range(256)], np.uint8)
    t.setflags(write=False)
    return t


def interpret(occupancy, track_unknown_space=True, trinary_costmap=True, lethal_cost_threshold=100, unknown_cost_value=-1):
    """incomingMap's loop (:199-207): `unsigned char value = new_map->data[index]` reads the int8 as its bit pattern"""
    occ = np.ascontiguousarray(occupancy, np.int8).view(np.uint8)
    return interpret_table(int(bool(track_unknown_space)), int(bool(trinary_costmap)), int(lethal_cost_threshold), int(unknown_cost_value))[occ]


# --------------------------------------------------------------------------------------------------------- merges
def _box(shape, box):
    ny, nx = shape
    return (0, 0, nx, ny) if box is None else tuple(int(v) for v in box)  # min_i, min_j, max_i, max_j


def reset_map(master, track_unknown, box=None):
    """costmap_2d.cpp:93-99: rows [y0, yn), columns [x0, xn) take default_value_ (255 with track_unknown, else 0)"""
    x0, y0, xn, yn = _box(master.shape, box)
    out = master.copy()
    out[y0:yn, x0:xn] = NO_INFORMATION if track_unknown else FREE_SPACE
    return out


def update_with_max(master, layer, box=None):
    """costmap_layer.cpp:62-86: a NO_INFORMATION layer cell is skipped; else the layer cell is taken where the master is
    NO_INFORMATION or lower"""
    x0, y0, xn, yn = _box(master.shape, box)
    out = master.copy()
    m, c = out[y0:yn, x0:xn], layer[y0:yn, x0:xn]
    take = (c != NO_INFORMATION) & ((m == NO_INFORMATION) | (m < c))
    m[take] = c[take]
    return out


def update_with_true_overwrite(master, layer, box=None):
    """costmap_layer.cpp:88-105"""
    x0, y0, xn, yn = _box(master.shape, box)
    out = master.copy()
    out[y0:yn, x0:xn] = layer[y0:yn, x0:xn]
    return out


def update_with_overwrite(master, layer, box=None):
    """costmap_layer.cpp:107-124"""
    x0, y0, xn, yn = _box(master.shape, box)
    out = master.copy()
    m, c = out[y0:yn, x0:xn], layer[y0:yn, x0:xn]
    take = c != NO_INFORMATION
    m[take] = c[take]
    return out


def static_update_costs(master, static, use_maximum, rolling=False, box=None):
    """static_layer.cpp:287-337.  rolling: the static map has the master's geometry and the transform is the identity, so
    worldToMap (:327) gives every master cell its own static cell and :329-332 is a plain copy or a plain std::max."""
    if not rolling:
        return update_with_max(master, static, box) if use_maximum else update_with_true_overwrite(master, static, box)
    x0, y0, xn, yn = _box(master.shape, box)
    out = master.copy()
    m, c = out[y0:yn, x0:xn], static[y0:yn, x0:xn]
    m[...] = np.maximum(c, m) if use_maximum else c
    return out


def obstacle_update_costs(master, layer, combination_method, box=None):
    """obstacle_layer.cpp:437-447: 0 updateWithOverwrite, 1 updateWithMax, anything else nothing"""
    if combination_method == 0:
        return update_with_overwrite(master, layer, box)
    if combination_method == 1:
        return update_with_max(master, layer, box)
    return master.copy()


def update_map(master, track_unknown, static, use_maximum, obstacle, combination_method, rolling_static=False, box=None):
    """layered_costmap.cpp:137-146: resetMap over the box, then every plugin's updateCosts in order (static, obstacle);
    `static` / `obstacle` None: that layer is absent"""
    out = reset_map(np.ascontiguousarray(master, np.uint8), track_unknown, box)
    if static is not None:
        out = static_update_costs(out, static, use_maximum, rolling_static, box)
    if obstacle is not None:
        out = obstacle_update_costs(out, obstacle, combination_method, box)
    return out


# --------------------------------------------------------------------------------------------------------- navfn
COST_UNKNOWN_ROS, COST_OBS, COST_OBS_ROS, COST_NEUTRAL, COST_FACTOR = 255, 254, 253, 50, 0.8  # navfn.h:49-67


def navfn_costarr(cmap, cost_mode, allow_unknown):
    """navfn.cpp:227-287 cell by cell.  cost_mode 1: isROS = true, 2: isROS = false (the PGM branch: a frame of 7 cells stays
    COST_OBS, unknown is passable whatever allow_unknown says), 0: the bytes are costarr itself (path_calc_test.cpp:52)"""
    cmap = np.ascontiguousarray(cmap, np.uint8)
    if cost_mode == 0:
        return cmap.copy()
    ny, nx = cmap.shape
    out = np.empty_like(cmap)
    for i in range(ny):
        for j in range(nx):
            cm = COST_OBS
            if cost_mode == 2 and (i < 7 or i > ny - 8 or j < 7 or j > nx - 8):
                out[i, j] = cm
                continue  # don't do borders
            v = int(cmap[i, j])
            if v < COST_OBS_ROS:
                v = int(COST_NEUTRAL + COST_FACTOR * v)  # int v = COST_NEUTRAL+COST_FACTOR*v: double, truncated
                if v >= COST_OBS:
                    v = COST_OBS - 1
                cm = v
            elif v == COST_UNKNOWN_ROS and (allow_unknown or cost_mode == 2):
                cm = COST_OBS - 1
            out[i, j] = cm
    return out


# --------------------------------------------------------------------------------------------------------- the tables
LETHAL_THRESHOLDS = tuple(range(101)) + (-7, 101, 127, 255, 256, 1000)  # every threshold, and six the clamp changes
UNKNOWN_COST_VALUES = (-1, 0, 1, 50, 99, 100, 128, 255, 256, -2, 511)   # wrap to a byte as the reference's assignment does


def static_parameter_table():
    """(track_unknown_space, trinary_costmap, lethal_cost_threshold, unknown_cost_value): 2 x 2 x 107 x 11 = 4708 settings"""
    return [(tu, tri, thr, unk) for thr in LETHAL_THRESHOLDS for unk in UNKNOWN_COST_VALUES for tri in (0, 1) for tu in (0, 1)]


def all_int8(ny, nx):
    """an occupancy grid whose cells are the 256 int8 bit patterns in order, repeated to fill ny x nx"""
    return (np.arange(ny * nx, dtype=np.uint32) & 0xFF).astype(np.uint8).view(np.int8).reshape(ny, nx)


def pair_tables(ny, nx):
    """two (ny, nx) uint8 grids holding the 65 536 byte pairs in row-major order, the remainder repeating: cell k pairs
    a = k & 255 with b = (k >> 8) & 255.  At 256 x 256 cell (y, x) pairs a = x with b = y."""
    k = np.arange(ny * nx, dtype=np.uint32)
    return (k & 0xFF).astype(np.uint8).reshape(ny, nx), ((k >> 8) & 0xFF).astype(np.uint8).reshape(ny, nx)


def navfn_byte_maps(ny, nx, count, step=18):
    """`count` (ny, nx) cost maps: map p holds byte (k + step p) & 255 in cell k, so that every byte reaches every cell
    class: the 18 = 2 x 9 cells that cost_mode 2's frame leaves of a 16 x 23 map see all 256 bytes within 16 maps of
    step 18, the single one of a 15 x 15 map within 256 maps of step 1 (the tests assert the coverage they rely on)"""
    k = np.arange(ny * nx, dtype=np.uint32).reshape(ny, nx)
    return np.stack([((k + step * p) & 0xFF).astype(np.uint8) for p in range(count)])


GEOMETRIES = [(256, 256), (263, 250)]  # (ny, nx) of the pair tables; nx = 250: k_merge's 16-cell groups straddle rows
NAVFN_SIZES = [(16, 23, 16, 18), (15, 15, 256, 1), (14, 30, 1, 18), (40, 33, 3, 18)]  # nx, ny, maps, byte step between maps


def rolling_occupancy(n):
    """column x holds the int8 bit pattern x: scaled with threshold 100 and unknown -1 that is 100 greys, 254 and 255"""
    return np.broadcast_to(np.arange(n, dtype=np.uint8).view(np.int8), (n, n)).copy()
