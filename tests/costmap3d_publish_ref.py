"""numpy restatement of costmap_3d's publishing as include/navgpu_costmap3d_publish.h states it, on top of the layered and rolling
yardsticks (tests/costmap3d_layers_ref.py, tests/costmap3d_rolling_ref.py): canonical pruning of a map into maximal octree leaves,
Costmap3DPublisher's full and delta messages with the diff bounds and the forgotten boxes, CostmapLayer3D::updateCells and
OctomapServerLayer3D's subscription state machine.

A volume is a uint8 array [x, y, z] of cell states (0 absent, 1 FREE, 2 NONLETHAL, 3 LETHAL) at a lattice origin ok; a leaf is the
tuple (kx, ky, kz, level, cls) with the C ABI's classes (LETHAL 0, NONLETHAL 1, FREE 2).  Pruning merges level by level on dense
arrays with plain comparisons: nothing here is a bit trick.  The closed forms in tests/test_costmap3d_publish_reference.py hold
this file in place."""
import numpy as np

import costmap3d_layers_ref as ref
import costmap3d_rolling_ref as rolling

CLS_LETHAL, CLS_NONLETHAL, CLS_FREE = 0, 1, 2
STATE_OF_CLS = {CLS_LETHAL: ref.LETHAL, CLS_NONLETHAL: ref.NONLETHAL, CLS_FREE: ref.FREE}
CLS_OF_STATE = {v: k for k, v in STATE_OF_CLS.items()}
FULL, DELTA = 0, 1
BINARY, AS_GIVEN = 0, 1
APPLIED, IGNORED, RESYNC = 0, 1, 2
MAX_LEVEL = 6


def prune(vol, ok, max_level=16):
    """the canonical prune of a volume of states at lattice origin ok: the set of maximal leaves (kx, ky, kz, level, cls).  A node
    becomes a leaf iff its 8 children are leaves of one class; what lies outside the volume is absent."""
    vol = np.asarray(vol, np.uint8)
    ok = [int(v) for v in ok]
    span = 1  # the largest node edge that fits the volume along every axis: no larger node can be full
    while span * 2 <= min(vol.shape) and span < (1 << max_level):
        span *= 2
    # the volume inside a dense array whose origin and size are multiples of span on the lattice
    lo = [o - o % span for o in ok]
    hi = [-((-(o + s)) // span) * span for o, s in zip(ok, vol.shape)]
    dense = np.zeros([h - l for l, h in zip(lo, hi)], np.uint8)
    dense[ok[0] - lo[0]:ok[0] - lo[0] + vol.shape[0], ok[1] - lo[1]:ok[1] - lo[1] + vol.shape[1], ok[2] - lo[2]:ok[2] - lo[2] + vol.shape[2]] = vol
    levels = [dense]  # levels[L][i, j, k]: the state of the node if it is a leaf (before maximality), else 0
    edge = 1
    while edge < span and edge < (1 << max_level):
        a = levels[-1]
        eight = a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2, a.shape[2] // 2, 2)
        smallest, largest = eight.min(axis=(1, 3, 5)), eight.max(axis=(1, 3, 5))
        levels.append(np.where(smallest == largest, smallest, 0).astype(np.uint8))
        edge *= 2
    leaves = set()
    for level, a in enumerate(levels):
        keep = a != 0
        if level + 1 < len(levels):  # not below a leaf
            keep &= np.repeat(np.repeat(np.repeat(levels[level + 1], 2, 0), 2, 1), 2, 2) == 0
        for i, j, k in zip(*np.nonzero(keep)):
            leaves.add((lo[0] + (int(i) << level), lo[1] + (int(j) << level), lo[2] + (int(k) << level), level, CLS_OF_STATE[int(a[i, j, k])]))
    return leaves


def prune_cells(cells, cls=CLS_LETHAL):
    """the prune of a list of lattice cells (n, 3) of one class"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    lo = cells.min(0)
    vol = np.zeros(cells.max(0) - lo + 1, np.uint8)
    vol[tuple((cells - lo).T)] = STATE_OF_CLS[cls]
    return prune(vol, lo)


def leaves_volume(leaves, ok, size, binary=False):
    """the cells of a set of leaves inside the window (ok, size): a volume of states, the higher class winning; binary: a bool mask"""
    vol = np.zeros(size, np.uint8)
    for kx, ky, kz, level, cls in leaves:
        edge = 1 << level
        lo = [max(k - o, 0) for k, o in zip((kx, ky, kz), ok)]
        hi = [min(k - o + edge, s) for k, o, s in zip((kx, ky, kz), ok, size)]
        if any(l >= h for l, h in zip(lo, hi)):
            continue
        part = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        np.maximum(part, 1 if binary else STATE_OF_CLS[cls], out=part)
    return vol.astype(bool) if binary else vol


def shadow_at(shadow, shadow_ok, ok, size):
    """the shadow read at the window (ok, size): each cell at its lattice position, absent outside the shadow's window"""
    out = np.zeros(size, np.uint8)
    if shadow is None:
        return out
    d = [int(a - b) for a, b in zip(ok, shadow_ok)]  # shadow index = window index + d
    lo = [max(0, -v) for v in d]
    hi = [min(s, t - v) for s, t, v in zip(size, shadow.shape, d)]
    if all(l < h for l, h in zip(lo, hi)):
        out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = shadow[lo[0] + d[0]:hi[0] + d[0], lo[1] + d[1]:hi[1] + d[1], lo[2] + d[2]:hi[2] + d[2]]
    return out


def forgotten_boxes(shadow_ok, ok, size):
    """shadow window minus current window as at most two inclusive lattice boxes (min xyz, max xyz): the x strip over the old y
    range, then the y strip over the remaining x range; both over the shadow window's z range"""
    sx, sy, sz = [int(v) for v in shadow_ok]
    cx, cy = int(ok[0]), int(ok[1])
    boxes = []
    xs = [x for x in range(sx, sx + size[0]) if not cx <= x < cx + size[0]]
    if xs:
        boxes.append((min(xs), sy, sz, max(xs), sy + size[1] - 1, sz + size[2] - 1))
    both = [x for x in range(sx, sx + size[0]) if cx <= x < cx + size[0]]
    ys = [y for y in range(sy, sy + size[1]) if not cy <= y < cy + size[1]]
    if both and ys:
        boxes.append((min(both), min(ys), sz, max(both), max(ys), sz + size[2] - 1))
    return boxes


class Publisher:
    """Costmap3DPublisher for one instance: the shadow, its window and update_seq"""

    def __init__(self):
        self.shadow, self.shadow_ok, self.seq = None, None, 0

    def full(self, master, ok):
        return dict(update_seq=self.seq, bounds_seq=(self.seq - 1) % (1 << 32), universe=1, values=prune(master, ok), bounds=set(), forgotten=[])

    def delta(self, master, ok):
        master = np.asarray(master, np.uint8)
        was = shadow_at(self.shadow, self.shadow_ok, ok, master.shape)
        differs = master != was
        msg = dict(update_seq=self.seq, bounds_seq=self.seq, universe=0, values=prune(np.where(differs, master, 0), ok),
                   bounds={l[:4] + (CLS_LETHAL,) for l in prune(np.where(differs, ref.LETHAL, 0), ok)},
                   forgotten=[] if self.shadow is None else forgotten_boxes(self.shadow_ok, ok, master.shape))
        self.shadow, self.shadow_ok, self.seq = master.copy(), [int(v) for v in ok], (self.seq + 1) % (1 << 32)
        return msg


def update_cells(vol, changed, ok, msg, cell_mode=BINARY):
    """CostmapLayer3D::updateCells on one layer's volume and changed mask, in place: erase inside the bounds, then set"""
    size = vol.shape
    if msg.get("universe") or msg.get("plain_map"):
        E = np.ones(size, bool)
    else:
        E = leaves_volume(msg.get("bounds", ()), ok, size, binary=True)
        for b in msg.get("forgotten", ()):
            E |= leaves_volume_box(b, ok, size)
    values = msg["values"]
    if cell_mode == BINARY:
        values = {l[:4] + (CLS_LETHAL if l[4] in (CLS_LETHAL, CLS_NONLETHAL) else CLS_FREE,) for l in values}
    V = leaves_volume(values, ok, size)
    vol[E] = V[E]
    changed |= E
    return E


def leaves_volume_box(box, ok, size):
    out = np.zeros(size, bool)
    lo = [max(box[a] - int(ok[a]), 0) for a in range(3)]
    hi = [min(box[3 + a] - int(ok[a]) + 1, size[a]) for a in range(3)]
    if all(l < h for l, h in zip(lo, hi)):
        out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return out


class Subscription:
    """OctomapServerLayer3D's state per (instance, layer): mapCallback / mapUpdateCallback (octomap_server_layer_3d.cpp:281-350)"""

    def __init__(self):
        self.using_updates = False
        self.resubscribe()

    def resubscribe(self):  # subscribeUpdatesUnlocked
        self.first_full, self.n_updates = False, 0

    def verdict(self, update_seq=0, bounds_seq=0, plain_map=False):
        if plain_map:
            return IGNORED if self.using_updates else APPLIED
        self.n_updates += 1
        if not self.first_full:
            if self.n_updates == 1 and bounds_seq == update_seq:
                return IGNORED
            if self.n_updates > 1:
                self.resubscribe()
                return RESYNC
            self.first_full = True
        elif (self.last_seq + 1) % (1 << 32) < bounds_seq:
            self.resubscribe()
            return RESYNC
        self.last_seq = bounds_seq
        self.using_updates = True
        return APPLIED


class PublishedMap(rolling.RollingMap):
    """a rolling layered map with a publisher on its master and fed layers"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.publisher = Publisher()

    def ok(self):
        return [int(v) for v in ref.origin_keys(self.origin, self.res)]

    def export(self, mode):
        return self.publisher.full(self.master, self.ok()) if mode == FULL else self.publisher.delta(self.master, self.ok())

    def feed(self, layer, msg, cell_mode=BINARY):
        return update_cells(self.vol[layer], self.changed[layer], self.ok(), msg, cell_mode)
