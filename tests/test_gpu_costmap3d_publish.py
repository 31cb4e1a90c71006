"""Publishing 3-D maps as pruned octree leaves and taking them in as a layer, on the device (include/navgpu_costmap3d_publish.h),
against the numpy yardstick (tests/costmap3d_publish_ref.py).  Everything the feature computes is integers and bits, so every
comparison is equality: leaf arrays as sets (and their length: no leaf twice), planes, `changed`, message fields.

Map P is 136 x 72 x 64 cells of 0.25 m at lattice origin (-13, 5, 0): x spans three 64-blocks of the lattice and starts on an odd
key, y spans two, z can hold a level-6 node.  Map Q is the same with lattice z origin -3, so z pairs do not start at bit 0.  The
aisles map is the reference's own octree file.  The yardstick's input for an export is the master as downloaded from the device
(the existing raw column calls), beside closed-form expectations where a case has one."""
import os

import numpy as np
import pytest

import costmap3d_layers_ref as ref
import costmap3d_publish_ref as pub

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")
RES = 0.25
SIZE = (136, 72, 64)
P_OK, Q_OK = (-13, 5, 0), (-13, 5, -3)
L, N, F = pub.CLS_LETHAL, pub.CLS_NONLETHAL, pub.CLS_FREE
XYZI = dict(kind=ref.POINT_CLOUD, cloud_has_intensity=1, free_intensity=0.25, lethal_intensity=0.75, max_cloud_points=4096)
FED = dict(kind=ref.POINT_CLOUD, max_cloud_points=1)
INTENSITY = {ref.FREE: 0.0, ref.NONLETHAL: 0.5, ref.LETHAL: 1.0}
POSE = [[0.0, 0.0, 0.0]]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def origin_of(ok):
    return np.asarray(ok, np.float64) * RES


def handle(nav, ok=P_OK, n=1, layers=None, size=SIZE, publisher=True, max_boxes=1 << 16):
    c3 = nav.Costmap3D(n, size[0], size[1], size[2], RES, max_triangles=1, max_boxes=max_boxes, max_poses=1)
    for i in range(n):
        c3.set_origin(i, origin_of(ok))
    if layers:
        c3.configure_layers(layers)
    if publisher:
        c3.configure_publisher()
    return c3


def put(c3, instance, vol):
    """a volume of LETHAL / NONLETHAL states straight into the master's planes"""
    c3.set_columns(instance, ref.to_words(vol, ref.LETHAL), ref.to_words(vol, ref.NONLETHAL))


def volume_of(lethal, nonlethal, free, sz):
    vol = np.zeros((lethal.shape[1], lethal.shape[0], sz), np.uint8)
    for z in range(sz):
        for plane, state in ((free, ref.FREE), (nonlethal, ref.NONLETHAL), (lethal, ref.LETHAL)):
            vol[:, :, z][((plane >> np.uint64(z)) & np.uint64(1)).T.astype(bool)] = state
    return vol


def master_of(c3, instance, layered):
    lethal, nonlethal = c3.columns(instance)
    free = c3.free_columns(instance) if layered else np.zeros_like(lethal)
    return volume_of(lethal, nonlethal, free, c3.size_z)


def leafset(a):
    out = {(int(l["key"][0]), int(l["key"][1]), int(l["key"][2]), int(l["level"]), int(l["cls"])) for l in a}
    assert len(out) == len(a), "a leaf is there twice"
    return out


def leaf_array(leaves):
    from navigation_amd.costmap3d import LEAF_DTYPE
    out = np.zeros(len(leaves), LEAF_DTYPE)
    for k, l in enumerate(sorted(leaves)):
        out[k] = (l[:3], l[3], l[4])
    return out


def parts(msgs, values, bounds, k):
    m = msgs[k]
    return values[m["first_value"]:m["first_value"] + m["n_values"]], bounds[m["first_bound"]:m["first_bound"] + m["n_bounds"]]


def full_of(c3, instance=0):
    msgs, values, bounds = c3.export([instance], 0)
    assert len(bounds) == 0 and msgs[0]["universe"] == 1 and msgs[0]["n_forgotten"] == 0 and msgs[0]["instance"] == instance
    assert (msgs[0]["first_value"], msgs[0]["n_values"]) == (0, len(values))
    return leafset(values)


def by_level(leaves):
    n = {}
    for l in leaves:
        n[l[3]] = n.get(l[3], 0) + 1
    return n


def cells_volume(cells, state=ref.LETHAL):
    vol = np.zeros(SIZE, np.uint8)
    for c in cells:
        vol[tuple(c)] = state
    return vol


@pytest.mark.parametrize("ok", [P_OK, Q_OK])
def test_full_single_cells_at_corners_and_block_borders(nav, ok):
    c3 = handle(nav, ok)
    corners = [(x, y, z) for x in (0, SIZE[0] - 1) for y in (0, SIZE[1] - 1) for z in (0, SIZE[2] - 1)]
    borders = [(k - ok[0], 30, 17) for k in (-1, 0, 63, 64)] + [(40, k - ok[1], 5) for k in (63, 64)]
    vol = cells_volume(corners + borders)
    put(c3, 0, vol)
    got = full_of(c3)
    assert got == {(ok[0] + x, ok[1] + y, ok[2] + z, 0, L) for x, y, z in corners + borders} == pub.prune(vol, ok)
    c3.close()


@pytest.mark.parametrize("ok", [P_OK, Q_OK])
def test_full_a_block_merges_only_where_the_lattice_has_a_node(nav, ok):
    c3 = handle(nav, ok)
    base = (20 - ok[0], 10 - ok[1], 8 - ok[2])  # lattice (20, 10, 8): a multiple of 2 on every axis
    for shift in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        vol = np.zeros(SIZE, np.uint8)
        x, y, z = (b + s for b, s in zip(base, shift))
        vol[x:x + 2, y:y + 2, z:z + 2] = ref.LETHAL
        put(c3, 0, vol)
        got = full_of(c3)
        assert got == pub.prune(vol, ok)
        assert by_level(got) == ({1: 1} if shift == (0, 0, 0) else {0: 8})
    if ok == Q_OK:  # bits 3..4 are lattice z 0..1, a node; bits 2..3 are lattice z -1..0, none
        for z0, want in ((3, {1: 1}), (2, {0: 8})):
            vol = np.zeros(SIZE, np.uint8)
            vol[base[0]:base[0] + 2, base[1]:base[1] + 2, z0:z0 + 2] = ref.LETHAL
            put(c3, 0, vol)
            assert by_level(full_of(c3)) == want
    c3.close()


def test_full_the_cube(nav):
    c3 = handle(nav)
    x0 = 0 - P_OK[0]  # lattice x 0..63 over the window's 72 rows, lattice y 5..76
    vol = np.zeros(SIZE, np.uint8)
    vol[x0:x0 + 64, :, :] = ref.LETHAL
    put(c3, 0, vol)
    got = full_of(c3)
    assert got == pub.prune(vol, P_OK) and max(by_level(got)) == 5  # the window is 72 rows: no level-6 node fits in y
    c3.close()
    # a window that holds a whole level-6 node: lattice x -13.., y -3..68
    ok = (-13, -3, 0)
    c3 = handle(nav, ok)
    x0, y0 = 0 - ok[0], 0 - ok[1]
    vol = np.zeros(SIZE, np.uint8)
    vol[x0:x0 + 64, y0:y0 + 64, :] = ref.LETHAL
    put(c3, 0, vol)
    assert full_of(c3) == {(0, 0, 0, 6, L)}
    for hole in ((0, 0, 0), (37, 21, 50)):
        less = vol.copy()
        less[x0 + hole[0], y0 + hole[1], hole[2]] = ref.ABSENT
        put(c3, 0, less)
        got = full_of(c3)
        assert by_level(got) == {l: 7 for l in range(6)} and got == pub.prune(less, ok)
    vol[:] = ref.ABSENT
    vol[x0 + 32:x0 + 96, y0:y0 + 64, :] = ref.LETHAL  # lattice x 32..95
    put(c3, 0, vol)
    got = full_of(c3)
    assert by_level(got) == {5: 8} and got == pub.prune(vol, ok)
    c3.close()


def cloud_of(vol, ok):
    """one xyzi point at the centre of every present cell"""
    xs, ys, zs = np.nonzero(vol)
    pts = np.zeros((len(xs), 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = [(np.asarray(c) + o + 0.5) * RES for c, o in zip((xs, ys, zs), ok)]
    pts[:, 3] = [INTENSITY[int(v)] for v in vol[xs, ys, zs]]
    return pts


def test_full_classes(nav):
    c3 = handle(nav, layers=[XYZI])
    vol = np.zeros(SIZE, np.uint8)
    vol[33:35, 11:13, 20:22] = ref.LETHAL      # lattice (20, 16, 20)
    vol[34, 11, 21] = ref.NONLETHAL
    vol[17:21, 3:7, 4:8] = ref.FREE            # lattice (4, 8, 4): a level-2 node
    vol[0, 1:3, 0:2] = ref.LETHAL              # lattice x -13, y 6..7: the parent overhangs the window
    vol[1:3, 1:3, 0:2] = ref.LETHAL            # lattice x -12, -11: a node
    pts = cloud_of(vol, P_OK)
    assert c3.buffer_clouds([(0, 0, 0, len(pts))], pts)[0] == 0
    c3.update([0], POSE)
    assert np.array_equal(master_of(c3, 0, True), vol)
    got = full_of(c3)
    assert got == pub.prune(vol, P_OK)
    assert (4, 8, 4, 2, F) in got and (-12, 6, 0, 1, L) in got and sum(l[0] == -13 for l in got) == 4 and sum(l[4] == N for l in got) == 1
    assert by_level(got) == {2: 1, 1: 1, 0: 12}
    c3.close()


def aisles_map(nav, n=1, **kw):
    from navigation_amd.costmap3d import read_octomap_bt
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    lo = (t["centres"] - 0.5 * t["sizes"][:, None]).min(0)
    hi = (t["centres"] + 0.5 * t["sizes"][:, None]).max(0)
    size = np.rint((hi - lo) / t["res"]).astype(int)
    c3 = nav.Costmap3D(n, int(size[0]), int(size[1]), int(size[2]), t["res"], max_triangles=1, max_boxes=1 << 16, max_poses=1, **kw)
    for i in range(n):
        c3.set_origin(i, lo)
        assert c3.set_boxes(i, t["centres"], t["sizes"]) == 0
    level = np.rint(np.log2(t["sizes"] / t["res"])).astype(int)
    key = np.rint((t["centres"] - 0.5 * t["sizes"][:, None]) / t["res"]).astype(int)
    return c3, {(int(k[0]), int(k[1]), int(k[2]), int(l), L) for k, l in zip(key, level)}


def test_full_on_the_aisles_map_is_the_files_leaves(nav):
    c3, file_leaves = aisles_map(nav, n=2)
    msgs, values, bounds = c3.export([0, 1], 0)
    assert by_level(file_leaves) == {0: 10421, 1: 33} and list(msgs["n_values"]) == [10454, 10454] and list(msgs["first_value"]) == [0, 10454]
    assert leafset(parts(msgs, values, bounds, 0)[0]) == leafset(parts(msgs, values, bounds, 1)[0]) == file_leaves
    assert (msgs["update_seq"] == 0).all() and (msgs["bounds_seq"] == 0).all()  # no publisher: no sequence numbers
    again = c3.export([0, 1], 0)
    assert values.tobytes() == again[1].tobytes() and msgs.tobytes() == again[0].tobytes()
    # the documented order inside an instance: by block, then class, then level coarse to fine, then key y, x, z
    v = parts(msgs, values, bounds, 0)[0]
    order = [(int(l["key"][1]) >> 6, int(l["key"][0]) >> 6, int(l["cls"]), -int(l["level"]), int(l["key"][1]), int(l["key"][0]), int(l["key"][2])) for l in v]
    assert order == sorted(order)
    c3.close()


def delta_of(c3, instance, p, layered):
    """one DELTA export of one instance against the yardstick's publisher p, fed the master as the device holds it"""
    ok = [int(v) for v in ref.origin_keys(c3.origin(instance), RES)]
    want = p.delta(master_of(c3, instance, layered), ok)
    msgs, values, bounds = c3.export([instance], 1)
    m = msgs[0]
    assert (m["update_seq"], m["bounds_seq"], m["universe"], m["plain_map"]) == (want["update_seq"], want["bounds_seq"], 0, 0)
    assert leafset(values) == want["values"] and leafset(bounds) == want["bounds"]
    assert [tuple(int(v) for v in b) for b in m["forgotten"][:m["n_forgotten"]]] == want["forgotten"]
    return msgs, values, bounds, want


def test_delta(nav):
    c3 = handle(nav, layers=[XYZI])
    p = pub.Publisher()
    vol = np.zeros(SIZE, np.uint8)
    vol[33:35, 11:13, 20:22] = ref.LETHAL
    vol[17:21, 3:7, 4:8] = ref.NONLETHAL       # lattice (4, 8, 4): a level-2 node
    vol[100, 60, 63] = ref.LETHAL
    pts = cloud_of(vol, P_OK)
    c3.buffer_clouds([(0, 0, 0, len(pts))], pts)
    c3.update([0], POSE)
    full = full_of(c3)
    _, _, _, first = delta_of(c3, 0, p, True)                                    # the first one: FULL's values, the bounds the present cells
    assert first["values"] == full and first["bounds"] == {l[:4] + (L,) for l in full} and first["update_seq"] == 0
    _, _, _, same = delta_of(c3, 0, p, True)                                     # unchanged: 0 / 0, the sequence number moves
    assert same["values"] == same["bounds"] == set() and same["update_seq"] == 1
    vol[100, 60, 63] = ref.FREE                                                  # one cell L -> F
    vol[17:21, 3:7, 4:8] = ref.ABSENT                                            # an aligned 4^3 block deleted
    pts = cloud_of(vol, P_OK)
    c3.buffer_clouds([(0, 0, 0, len(pts))], pts)
    c3.update([0], POSE)
    _, _, _, third = delta_of(c3, 0, p, True)
    assert third["values"] == {(87, 65, 63, 0, F)} and third["bounds"] == {(87, 65, 63, 0, L), (4, 8, 4, 2, L)} and third["update_seq"] == 2
    c3.set_boxes(0, [origin_of(P_OK) + (np.array([50, 20, 10]) + 1.0) * RES], 2 * RES, mode=1)   # MARK: past the layers
    _, _, _, marked = delta_of(c3, 0, p, True)
    assert by_level(marked["values"]) in ({1: 1}, {0: 8}) and len(marked["bounds"]) == len(marked["values"])
    c3.reset([0])
    _, _, _, gone = delta_of(c3, 0, p, True)
    assert gone["values"] == set() and gone["update_seq"] == 4 and pub.leaves_volume(gone["bounds"], P_OK, SIZE, binary=True).sum() == 8 + 8 + 1
    assert full_of(c3) == set()
    c3.close()


def test_delta_behind_a_roll(nav):
    c3 = handle(nav, layers=[XYZI])
    p = pub.Publisher()
    rng = np.random.default_rng(7)
    vol = np.zeros(SIZE, np.uint8)
    cells = np.stack([rng.integers(0, SIZE[0], 300), rng.integers(0, SIZE[1], 300), rng.integers(0, SIZE[2], 300)], 1)
    vol[tuple(cells.T)] = rng.choice([ref.FREE, ref.NONLETHAL, ref.LETHAL], 300)
    vol[0:2, 70:72, 0:2] = ref.LETHAL          # a corner that leaves with (+3, -2)
    pts = cloud_of(vol, P_OK)
    c3.buffer_clouds([(0, 0, 0, len(pts))], pts)
    c3.update([0], POSE)
    delta_of(c3, 0, p, True)
    ok = np.array(P_OK)
    for (dx, dy), boxes in (((3, -2), 2), ((-70, 0), 1), ((0, 0), 0), ((400, 9), 1)):
        ok = ok + (dx, dy, 0)
        shifts = c3.roll([0], origin_xy=[origin_of(ok)[:2]])
        assert tuple(shifts[0]) == (dx, dy)
        entering = np.zeros(SIZE, np.uint8)       # content in what entered: the cloud layer is replaced, so send what is there again too
        stayed = master_of(c3, 0, True)
        entering[5:9, 30:34, 8:12] = ref.NONLETHAL
        entering[stayed != ref.ABSENT] = stayed[stayed != ref.ABSENT]
        pts = cloud_of(entering, ok)
        c3.buffer_clouds([(0, 0, 0, len(pts))], pts)
        c3.update([0], POSE)
        msgs, values, bounds, want = delta_of(c3, 0, p, True)
        assert msgs[0]["n_forgotten"] == boxes
        now = master_of(c3, 0, True)
        in_bounds = pub.leaves_volume(leafset(bounds), ok, SIZE, binary=True)
        assert not (in_bounds & (now == stayed) & (stayed != ref.ABSENT)).any()   # cells that stayed are in no bound
        assert in_bounds[5:9, 30:34, 8:12].any() == (not np.array_equal(stayed[5:9, 30:34, 8:12], now[5:9, 30:34, 8:12]))
    c3.close()


def test_capacity_and_counting_commit_nothing(nav):
    c3 = handle(nav)
    vol = cells_volume([(3, 3, 3), (70, 40, 9), (135, 71, 63)])
    vol[20:22, 20:22, 20:22] = ref.NONLETHAL
    put(c3, 0, vol)
    from navigation_amd.costmap3d import LEAF_DTYPE, UPDATE_MSG_DTYPE
    lib, ins = c3.L, np.zeros(1, np.uint32)
    want_n = len(pub.prune(vol, P_OK))
    vp = lambda a: a.ctypes.data
    for mode in (0, 1):
        msgs, short, room = np.zeros(1, UPDATE_MSG_DTYPE), np.zeros(want_n, LEAF_DTYPE), np.zeros(want_n, LEAF_DTYPE)
        short[:] = ((7, 7, 7), 7, 7)
        assert lib.navgpu_costmap3d_export(c3.h, 1, vp(ins), mode, want_n - 1, vp(short), want_n, vp(room), vp(msgs)) == -4
        assert msgs[0]["n_values"] == want_n and msgs[0]["n_bounds"] == (want_n if mode else 0) and (short["level"] == 7).all()
        counted = c3.export_counts([0], mode)
        assert counted.tobytes() == msgs.tobytes() and counted[0]["update_seq"] == 0
    msgs, values, bounds = c3.export([0], 1)     # with room: the same message, the same sequence number
    assert msgs.tobytes() == counted.tobytes() and leafset(values) == pub.prune(vol, P_OK)
    assert c3.export([0], 1)[0][0]["update_seq"] == 1 and c3.export_counts([0], 1)[0]["n_bounds"] == 0
    c3.close()


def test_a_mixed_list_leaves_the_unlisted_instance_alone(nav):
    c3 = handle(nav, n=3)
    vols = []
    for i in range(3):
        vol = cells_volume([(3 + i, 3, 3), (70, 40 + i, 9)])
        vol[64 + 2 * i:66 + 2 * i, 20:22, 20:22] = ref.LETHAL
        vols.append(vol)
        put(c3, i, vol)
    msgs, values, bounds = c3.export([2, 0], 1)
    assert list(msgs["instance"]) == [2, 0] and list(msgs["first_value"]) == [0, msgs[0]["n_values"]]
    for k, i in enumerate((2, 0)):
        v, b = parts(msgs, values, bounds, k)
        assert leafset(v) == pub.prune(vols[i], P_OK) and leafset(b) == leafset(v)
    msgs, values, bounds = c3.export([0, 1, 2], 1)
    assert list(msgs["update_seq"]) == [1, 0, 1] and list(msgs["n_values"]) == [0, len(pub.prune(vols[1], P_OK)), 0]
    assert leafset(values) == pub.prune(vols[1], P_OK)
    c3.close()


def msg_of(instance, seqs, values, bounds=(), universe=0, plain_map=0, forgotten=()):
    from navigation_amd.costmap3d import UPDATE_MSG_DTYPE
    m = np.zeros(1, UPDATE_MSG_DTYPE)
    m["instance"], m["update_seq"], m["bounds_seq"], m["universe"], m["plain_map"] = instance, seqs[0], seqs[1], universe, plain_map
    m["n_values"], m["n_bounds"], m["n_forgotten"] = len(values), len(bounds), len(forgotten)
    for k, b in enumerate(forgotten):
        m["forgotten"][0, k] = b
    return m


def layer_state(c3, instance, layer):
    lethal, nonlethal, free, changed = c3.layer_columns(instance, layer)
    return volume_of(lethal, nonlethal, free, c3.size_z), volume_of(changed, np.zeros_like(changed), np.zeros_like(changed), c3.size_z) == ref.LETHAL


UPDATE_CASES = {
    "levels": dict(bounds={(20, 10, 8, 0, L), (22, 10, 8, 1, L), (24, 16, 8, 3, L), (0, 0, 0, 6, L)},
                   values={(20, 10, 8, 0, F), (22, 10, 8, 1, N), (24, 16, 8, 3, L), (64, 64, 0, 6, L), (0, 0, 0, 5, N)}),
    "clipped": dict(bounds={(-16, 0, 0, 3, L), (120, 72, 56, 3, L), (-64, 64, 0, 6, L), (64, 0, 0, 6, L)},
                    values={(-16, 0, 0, 3, L), (120, 72, 56, 3, F), (-64, 64, 0, 6, N), (64, 0, 0, 6, L)}),
    "universe": dict(universe=1, values={(0, 8, 0, 3, L), (-13, 5, 0, 0, F)}),
    "plain": dict(plain_map=1, values={(0, 8, 0, 3, N)}),
    "forgotten": dict(bounds={(30, 30, 30, 0, L)}, values={(30, 30, 30, 0, L), (-10, 10, 0, 1, L)}, forgotten=[(-13, 5, 0, -9, 76, 63), (-8, 5, 0, 122, 6, 63)]),
    "two classes": dict(bounds={(16, 16, 16, 2, L)}, values={(16, 16, 16, 2, F), (16, 16, 16, 1, L), (18, 18, 18, 0, N), (16, 16, 16, 0, N)}),
}


@pytest.mark.parametrize("mode", [pub.BINARY, pub.AS_GIVEN])
@pytest.mark.parametrize("case", sorted(UPDATE_CASES))
def test_update_cells(nav, case, mode):
    spec = UPDATE_CASES[case]
    layers = [dict(XYZI), dict(FED)]
    c3 = handle(nav, layers=layers, publisher=False)
    m = pub.PublishedMap(SIZE, origin_of(P_OK), RES, layers)
    # what the fed layer holds before: cells in tiles (row 40, columns 51..) that the message does not touch, and some it erases
    before = [(-13 + x, 5 + y, z, 0, L) for x, y, z in ((60, 40, 1), (64, 40, 2), (135, 40, 63), (33, 5, 8), (29, 11, 8), (43, 25, 30))]
    first = dict(universe=1, values=set(before))
    assert c3.update_cells(msg_of(0, (1, 0), before, universe=1), [1], leaf_array(before), cell_mode=mode)[0] == pub.APPLIED
    m.feed(1, first, mode)
    c3.update([0], POSE)
    m.update(POSE[0])
    values, bounds = spec["values"], spec.get("bounds", set())
    msg = msg_of(0, (1, 1), values, bounds, spec.get("universe", 0), spec.get("plain_map", 0), spec.get("forgotten", ()))
    verdict = c3.update_cells(msg, [1], leaf_array(values), leaf_array(bounds), cell_mode=mode)[0]
    if spec.get("plain_map"):
        assert verdict == pub.IGNORED        # updates are in use on this pair
        c3.resubscribe(0, 1)
        c3.close()
        c3 = handle(nav, layers=layers, publisher=False)
        m = pub.PublishedMap(SIZE, origin_of(P_OK), RES, layers)
        assert c3.update_cells(msg, [1], leaf_array(values), cell_mode=mode)[0] == pub.APPLIED
    else:
        assert verdict == pub.APPLIED
    E = m.feed(1, dict(spec, values=values, bounds=bounds), mode)
    vol, changed = layer_state(c3, 0, 1)
    assert np.array_equal(vol, m.vol[1]) and np.array_equal(changed, m.changed[1]) and np.array_equal(changed, E)   # changed is E exactly
    c3.update([0], POSE)
    m.update(POSE[0])
    assert np.array_equal(master_of(c3, 0, True), m.master) and np.array_equal(c3.layer2d(0), m.layer2d)
    # the tile bitmaps: a cloud into tiles of the other layer that were empty, then an update, then a message into empty tiles of the fed one
    cloud = np.zeros(SIZE, np.uint8)
    cloud[2, 70, 3], cloud[130, 1, 60], cloud[70, 50, 9] = ref.LETHAL, ref.FREE, ref.NONLETHAL
    pts = cloud_of(cloud, P_OK)
    assert c3.buffer_clouds([(0, 0, 0, len(pts))], pts)[0] == 0 and m.buffer_cloud(0, pts) == 0
    late = {(-13 + 100, 5 + 66, 40, 0, N)}
    c3.update_cells(msg_of(0, (3, 2), late, late), [1], leaf_array(late), leaf_array(late), cell_mode=mode)
    m.feed(1, dict(values=late, bounds=late), mode)
    c3.update([0], POSE)
    m.update(POSE[0])
    assert np.array_equal(master_of(c3, 0, True), m.master)
    vol, changed = layer_state(c3, 0, 1)
    assert np.array_equal(vol, m.vol[1]) and not changed.any()
    c3.close()


def test_update_cells_for_a_list_of_pairs(nav):
    layers = [dict(FED), dict(FED)]
    c3 = handle(nav, n=2, layers=layers, publisher=False)
    maps = [pub.PublishedMap(SIZE, origin_of(P_OK), RES, layers) for _ in range(2)]
    from navigation_amd.costmap3d import UPDATE_MSG_DTYPE
    sets = [{(0, 8, 0, 3, L), (9, 9, 9, 0, F)}, {(64, 64, 0, 2, N)}, {(-12, 6, 2, 1, L), (-13, 5, 0, 0, N)}]
    pairs = [(1, 0), (0, 1), (1, 1)]
    msgs = np.concatenate([msg_of(i, (1, 0), s, universe=1) for (i, _), s in zip(pairs, sets)]).view(UPDATE_MSG_DTYPE)
    msgs["first_value"] = np.cumsum([0] + [len(s) for s in sets[:-1]])
    values = np.concatenate([leaf_array(s) for s in sets])
    assert list(c3.update_cells(msgs, [l for _, l in pairs], values, cell_mode=pub.AS_GIVEN)) == [pub.APPLIED] * 3
    for (i, l), s in zip(pairs, sets):
        maps[i].feed(l, dict(universe=1, values=s), pub.AS_GIVEN)
    c3.update([0, 1], POSE * 2)
    for i in range(2):
        maps[i].update(POSE[0])
        assert np.array_equal(master_of(c3, i, True), maps[i].master)
        for l in range(2):
            assert np.array_equal(layer_state(c3, i, l)[0], maps[i].vol[l])
    c3.close()


def test_mirror_chain(nav):
    """handle A: three layers, rolling; handle B: one fed layer in a standing window that contains A's.  After every cycle's DELTA ->
    update_cells(AS_GIVEN) -> update, B's master is A's master at its lattice position and nothing else."""
    size_a, size_b = (72, 40, 64), (136, 72, 64)
    ok_a, ok_b = np.array([3, 9, -3]), (-13, 5, -3)
    stack = [dict(kind=ref.STATIC_2D, height=-0.5, lethal_cost_threshold=100), dict(XYZI), dict(kind=ref.CYLINDER_CLEARING, radius=0.8)]
    a = handle(nav, ok_a, layers=stack, size=size_a)
    b = handle(nav, ok_b, layers=[dict(FED)], size=size_b, publisher=False)
    rng = np.random.default_rng(11)
    grid = rng.choice(np.array([-1, 0, 100], np.int8), (size_a[1], size_a[0]))
    a.set_static_grid(0, 0, grid, *origin_of(ok_a)[:2])
    msgs, values, bounds = a.export([0], 0)                                       # a subscriber starts with the full map
    assert b.update_cells(msgs, [0], values, bounds, cell_mode=pub.AS_GIVEN)[0] == pub.APPLIED
    rolls = [(0, 0), (5, -3), (0, 0), (-9, 2), (30, 10), (0, 0)]
    for cycle, (dx, dy) in enumerate(rolls):
        ok_a = ok_a + (dx, dy, 0)
        a.roll([0], origin_xy=[origin_of(ok_a)[:2]])
        cells = np.stack([rng.integers(0, size_a[0], 200), rng.integers(0, size_a[1], 200), rng.integers(0, 64, 200)], 1)
        cloud = np.zeros(size_a, np.uint8)
        cloud[tuple(cells.T)] = rng.choice([ref.FREE, ref.NONLETHAL, ref.LETHAL], 200)
        cloud[8:16, 8:16, 11:19] = ref.LETHAL                                       # something that prunes: lattice z 8..15
        pts = cloud_of(cloud, ok_a)
        a.buffer_clouds([(0, 1, 0, len(pts))], pts)
        if cycle == 2:
            lo = origin_of(ok_a) + np.array([4, 4, 0]) * RES
            a.reset_bounding_box([0], [list(lo) + list(lo + 20 * RES)], [1])
        a.update([0], [list(origin_of(ok_a)[:2] + (4.0 + cycle, 3.0)) + [0.0]])
        if cycle == 3:
            a.set_boxes(0, [origin_of(ok_a) + (np.array([40, 20, 30]) + 2.0) * RES], 4 * RES, mode=1)
        msgs, values, bounds = a.export([0], 1)
        assert msgs[0]["update_seq"] == cycle and msgs[0]["n_forgotten"] == (0 if (dx, dy) == (0, 0) else 2)
        assert b.update_cells(msgs, [0], values, bounds, cell_mode=pub.AS_GIVEN)[0] == pub.APPLIED
        b.update([0], POSE)
        want = np.zeros(size_b, np.uint8)
        d = ok_a - np.array(ok_b)
        want[d[0]:d[0] + size_a[0], d[1]:d[1] + size_a[1], :] = master_of(a, 0, True)
        assert np.array_equal(master_of(b, 0, True), want), cycle
    assert len({int(v) for v in np.unique(want)}) == 4                             # all three classes and absent took part
    a.close()
    b.close()
