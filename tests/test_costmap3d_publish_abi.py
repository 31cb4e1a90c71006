"""CPU-side checks of the publishing C-ABI (include/navgpu_costmap3d_publish.h, included by navgpu.h): the record layouts and constants
agree with the header as the C compiler sees it; the four entry points are declared in that header only, exported, bound and each
cites the reference lines it replaces; every argument error is found on the host, before a device is opened; the subscription
verdicts come from the host alone - so all of this gives the same answers on a machine without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("navgpu_costmap3d_publisher_configure", "navgpu_costmap3d_export", "navgpu_costmap3d_layer_update_cells", "navgpu_costmap3d_layer_resubscribe")
INVALID, NO_DEVICE, CAPACITY, STATE = -1, -2, -4, -5
FULL, DELTA = 0, 1
BINARY, AS_GIVEN = 0, 1
APPLIED, IGNORED, RESYNC = 0, 1, 2
STACK = (dict(kind=1, height=0.0, lethal_cost_threshold=100), dict(kind=0, max_cloud_points=1), dict(kind=2, radius=0.5))
ALIGNED = np.array([-2.0, 1.0, -0.5])


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def u32(*v):
    return np.array(v, np.uint32)


def make(nav, layered=True, **kw):
    from navigation_amd import _lib
    d = dict(n_instances=3, size_x=16, size_y=8, size_z=64, resolution=0.25, max_triangles=4, max_boxes=8, max_poses=4, device=0)
    d.update(kw)
    h = C.c_void_p()
    L = nav.lib()
    assert L.navgpu_costmap3d_create(C.byref(_lib.Costmap3DDesc(**d)), C.byref(h)) == 0
    for i in range(d["n_instances"]):
        assert L.navgpu_costmap3d_set_origin(h, i, vp(ALIGNED)) == 0
    if layered:
        recs = (_lib.C3dLayer * len(STACK))()
        for k, s in enumerate(STACK):
            recs[k] = _lib.C3dLayer(**dict(dict(enabled=1, combination_method=1, max_cloud_points=8), **s))
        assert L.navgpu_costmap3d_configure_layers(h, recs, len(STACK), 127) == 0
    return h


def messages(n=1, **fields):
    from navigation_amd.costmap3d import UPDATE_MSG_DTYPE
    m = np.zeros(n, UPDATE_MSG_DTYPE)
    for k, v in fields.items():
        m[k] = v
    return m


def leaves(*rows):
    from navigation_amd.costmap3d import LEAF_DTYPE
    out = np.zeros(len(rows), LEAF_DTYPE)
    for k, (key, level, cls) in enumerate(rows):
        out[k] = (key, level, cls)
    return out


def test_records_and_constants_match_the_header(tmp_path):
    from navigation_amd import _lib, costmap3d
    fields = ("instance", "update_seq", "bounds_seq", "universe", "plain_map", "first_value", "n_values", "first_bound", "n_bounds", "n_forgotten", "forgotten")
    src = tmp_path / "consts.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "navgpu.h"\nint main(){printf("%d %d %d %d %d %d %d %d %d %d %d ", (int)NAVGPU_C3D_LETHAL, '
                   '(int)NAVGPU_C3D_NONLETHAL, (int)NAVGPU_C3D_FREE, (int)NAVGPU_C3D_EXPORT_FULL, (int)NAVGPU_C3D_EXPORT_DELTA, (int)NAVGPU_C3D_CELLS_BINARY, '
                   '(int)NAVGPU_C3D_CELLS_AS_GIVEN, (int)NAVGPU_C3D_APPLIED, (int)NAVGPU_C3D_IGNORED, (int)NAVGPU_C3D_RESYNC, 0);'
                   'printf("%d %d %d %d %d ", (int)sizeof(navgpu_c3d_leaf), (int)offsetof(navgpu_c3d_leaf, level), (int)offsetof(navgpu_c3d_leaf, cls), '
                   '(int)sizeof(navgpu_c3d_update_msg), 0);'
                   + "".join(f'printf("%d ", (int)offsetof(navgpu_c3d_update_msg, {f}));' for f in fields) + 'return 0;}\n')
    exe = tmp_path / "consts"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:11] == [_lib.C3D_LETHAL, _lib.C3D_NONLETHAL, _lib.C3D_FREE, _lib.C3D_EXPORT_FULL, _lib.C3D_EXPORT_DELTA, _lib.C3D_CELLS_BINARY, _lib.C3D_CELLS_AS_GIVEN,
                        _lib.C3D_APPLIED, _lib.C3D_IGNORED, _lib.C3D_RESYNC, 0] == [0, 1, 2, 0, 1, 0, 1, 0, 1, 2, 0]
    assert out[11:16] == [16, 12, 14, 88, 0]
    assert C.sizeof(_lib.C3dLeaf) == costmap3d.LEAF_DTYPE.itemsize == 16 and C.sizeof(_lib.C3dUpdateMsg) == costmap3d.UPDATE_MSG_DTYPE.itemsize == 88
    for f, offset in zip(fields, out[16:]):
        assert getattr(_lib.C3dUpdateMsg, f).offset == offset == costmap3d.UPDATE_MSG_DTYPE.fields[f][1], f
    assert (_lib.C3dLeaf.level.offset, _lib.C3dLeaf.cls.offset) == (12, 14) == (costmap3d.LEAF_DTYPE.fields["level"][1], costmap3d.LEAF_DTYPE.fields["cls"][1])


def test_entry_points_are_declared_exported_bound_and_cite_the_reference(nav):
    from navigation_amd import _lib
    L = nav.lib()
    main = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    assert '#include "navgpu_costmap3d_publish.h"' in main
    header = open(os.path.join(ROOT, "include", "navgpu_costmap3d_publish.h")).read()
    others = [open(os.path.join(ROOT, "include", f)).read() for f in ("navgpu_costmap3d_layers.h", "navgpu_costmap3d_rolling.h")]
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ENTRY_POINTS:
        m = re.search(r"\bint " + name + r"\(", header)
        assert m, name
        assert not re.search(r"\b" + name + r"\s*\(", main) and not any(re.search(r"\bint " + name + r"\(", o) for o in others), name
        assert hasattr(L, name) and name in bound, name
        comment = header[header.rindex("/*", 0, m.start()):header.rindex("*/", 0, m.start())]
        assert re.search(r"\w+\.(cpp|h):\d+(-\d+)?", comment), name
    assert set(re.findall(r"\bint (navgpu_costmap3d_\w+)\(", header)) == set(ENTRY_POINTS)
    for method in ("configure_publisher", "export", "update_cells", "resubscribe"):
        assert callable(getattr(nav.Costmap3D, method))


def test_null_handles(nav):
    L = nav.lib()
    p = vp(np.zeros(32))
    assert L.navgpu_costmap3d_publisher_configure(None, 1) == INVALID
    assert L.navgpu_costmap3d_export(None, 0, p, FULL, 0, None, 0, None, p) == INVALID
    assert L.navgpu_costmap3d_layer_update_cells(None, 0, p, p, BINARY, None, 0, None, 0, None) == INVALID
    assert L.navgpu_costmap3d_layer_resubscribe(None, 0, 0) == INVALID


@pytest.mark.parametrize("layered", [False, True])
def test_export_argument_errors_need_no_gpu(nav, layered):
    L = nav.lib()
    h = make(nav, layered)
    msgs = messages(3)
    msgs["n_values"] = 77
    buf = leaves(*[((0, 0, 0), 0, 0)] * 4)
    export = lambda ins, mode=FULL, vc=4, v=buf, bc=4, b=buf, m=msgs: L.navgpu_costmap3d_export(h, len(ins), vp(ins), mode, vc, vp(v), bc, vp(b), vp(m))
    assert export(u32(3)) == INVALID and export(u32(1, 1)) == INVALID                                   # out of range, listed twice
    assert export(u32(0), mode=2) == INVALID and export(u32(0), mode=-1) == INVALID
    assert export(u32(0), m=None) == INVALID
    assert export(u32(0), v=None) == INVALID and export(u32(0), b=None) == INVALID                      # a NULL buffer with a capacity
    assert L.navgpu_costmap3d_export(h, 1, None, FULL, 0, None, 0, None, vp(msgs)) == INVALID
    assert export(u32(0), mode=DELTA) == STATE                                                          # before publisher_configure
    assert L.navgpu_costmap3d_set_origin(h, 1, vp(np.array([-2.0, 1.1, -0.5]))) == 0                   # an unaligned origin
    assert export(u32(0, 1)) == INVALID
    assert L.navgpu_costmap3d_set_origin(h, 1, vp(ALIGNED)) == 0
    assert L.navgpu_costmap3d_publisher_configure(h, 1) == 0
    assert export(u32()) == 0 and export(u32(), mode=DELTA) == 0                                        # an empty list needs no device
    assert (msgs["n_values"] == 77).all()                                                               # a call that fails writes nothing
    if L.navgpu_device_count() <= 0:  # what is valid needs the device: there is no CPU fallback
        assert export(u32(0, 2)) == NO_DEVICE and export(u32(1), mode=DELTA) == NO_DEVICE
        assert export(u32(0), vc=0, v=None, bc=0, b=None) == NO_DEVICE
    assert L.navgpu_costmap3d_publisher_configure(h, 0) == 0 and export(u32(0), mode=DELTA) == STATE
    assert L.navgpu_costmap3d_destroy(h) == 0


def test_update_cells_argument_errors_need_no_gpu(nav):
    L = nav.lib()
    ok = (-8, 4, -2)                                                                                     # ALIGNED / 0.25
    good = leaves(((-8, 4, -2), 1, 0), ((-7, 5, -1), 0, 2), ((-64, 0, -64), 6, 1))
    verdicts = np.full(4, 77, np.int32)

    def feed(h, m, lay=(1,), mode=BINARY, v=good, b=good, out=verdicts):
        lay = u32(*lay)
        return L.navgpu_costmap3d_layer_update_cells(h, len(m), vp(m), vp(lay), mode, vp(v), 0 if v is None else len(v), vp(b), 0 if b is None else len(b), vp(out))

    one = lambda **f: messages(1, **dict(dict(update_seq=1, bounds_seq=0, n_values=3, n_bounds=3), **f))
    h = make(nav, layered=False)
    assert feed(h, one()) == STATE                                                                      # before configure_layers
    assert L.navgpu_costmap3d_layer_resubscribe(h, 0, 1) == STATE
    assert L.navgpu_costmap3d_destroy(h) == 0
    h = make(nav)
    assert feed(h, one(), mode=2) == INVALID and feed(h, one(), mode=-1) == INVALID
    assert feed(h, one(instance=3)) == INVALID and feed(h, one(), lay=(3,)) == INVALID
    assert feed(h, one(), lay=(2,)) == INVALID                                                          # a cylinder layer
    assert L.navgpu_costmap3d_layer_resubscribe(h, 0, 2) == INVALID and L.navgpu_costmap3d_layer_resubscribe(h, 3, 1) == INVALID
    assert L.navgpu_costmap3d_layer_resubscribe(h, 0, 3) == INVALID
    assert feed(h, messages(2, update_seq=1), lay=(1, 1)) == INVALID                                    # a pair named twice
    assert feed(h, one(first_value=1)) == INVALID and feed(h, one(first_bound=2, n_bounds=2)) == INVALID  # ranges beyond the arrays
    assert feed(h, one(n_forgotten=3)) == INVALID
    inverted = one(n_forgotten=1)
    inverted["forgotten"][0, 0] = (0, 0, 0, 3, -1, 3)
    assert feed(h, inverted) == INVALID
    for bad in (((-7, 4, -2), 1, 0), ((-8, 4, -1), 1, 0), ((-8, 6, -4), 2, 0), ((0, 0, 0), 7, 0), ((0, 0, 0), 0, 3), ((32, 0, 0), 6, 0)):
        assert feed(h, one(n_values=1, n_bounds=0), v=leaves(bad)) == INVALID, bad                      # not aligned to its level, level > 6, a bad class
        assert feed(h, one(n_values=0, n_bounds=1), b=leaves(bad)) == INVALID, bad
    assert L.navgpu_costmap3d_layer_update_cells(h, 1, vp(one()), vp(u32(1)), BINARY, None, 3, vp(good), 3, None) == INVALID
    assert L.navgpu_costmap3d_layer_update_cells(h, 1, None, vp(u32(1)), BINARY, vp(good), 3, vp(good), 3, None) == INVALID
    assert L.navgpu_costmap3d_layer_update_cells(h, 1, vp(one()), None, BINARY, vp(good), 3, vp(good), 3, None) == INVALID
    many = leaves(*[((0, 0, 0), 0, 0)] * 5)
    assert feed(h, one(n_values=5, n_bounds=4), v=many, b=many) == CAPACITY                             # 5 + 5 > max_boxes = 8
    assert L.navgpu_costmap3d_set_origin(h, 0, vp(np.array([-2.0, 1.0, -0.45]))) == 0                  # an unaligned origin
    assert feed(h, one()) == INVALID
    assert L.navgpu_costmap3d_set_origin(h, 0, vp(ALIGNED)) == 0
    assert (verdicts == 77).all()                                                                       # a call that fails writes nothing
    assert L.navgpu_costmap3d_destroy(h) == 0
    assert ok == tuple(int(v) for v in np.rint(ALIGNED / 0.25))


def test_the_verdicts_come_from_the_host(nav):
    """IGNORED / RESYNC / backwards / the uint32_t wrap through the C ABI; a failing call moves no state; what is applied needs the
    device, what is not needs none"""
    L = nav.lib()
    h = make(nav)
    have_gpu = L.navgpu_device_count() > 0

    def feed(seqs, lay=1, instance=0, plain=0, universe=0):
        m = messages(1, instance=instance, update_seq=seqs[0], bounds_seq=seqs[1], plain_map=plain, universe=universe)
        out = np.full(1, 77, np.int32)
        rc = L.navgpu_costmap3d_layer_update_cells(h, 1, vp(m), vp(u32(lay)), BINARY, None, 0, None, 0, vp(out))
        return rc, int(out[0])

    applied = (0, APPLIED)                                   # an empty delta is applied and queues nothing: no device is needed
    assert feed((5, 5)) == (0, IGNORED)                      # the first message is a normal update
    assert feed((5, 4)) == (0, RESYNC)                       # the quirk: the next one always resubscribes
    assert feed((5, 5)) == (0, IGNORED) and feed((6, 6)) == (0, RESYNC)
    if not have_gpu:                                         # a full map has work for the device; the failed call moves no state
        assert feed((6, 5), universe=1) == (NO_DEVICE, 77) and feed((7, 7)) == (0, IGNORED) and feed((7, 7)) == (0, RESYNC)
    assert feed((6, 5)) == applied                           # the full map's sentinel
    assert feed((6, 6)) == applied and feed((7, 7)) == applied
    assert feed((0, 0), plain=1) == (0, IGNORED)             # updates are in use
    assert feed((3, 3)) == applied                           # backwards is applied
    assert feed((5, 5)) == (0, RESYNC)                       # 3 + 1 < 5
    assert feed((0, 0xFFFFFFFF)) == applied and feed((0, 0)) == applied   # the sentinel of a fresh publisher, then the wrap
    assert feed((2, 2)) == (0, RESYNC)
    assert feed((0, 0), lay=0, plain=1) == (applied if have_gpu else (NO_DEVICE, 77))   # another pair has its own state; a plain map is a whole map
    assert feed((9, 9), instance=1) == (0, IGNORED)
    assert L.navgpu_costmap3d_layer_resubscribe(h, 1, 1) == 0
    assert feed((9, 9), instance=1) == (0, IGNORED)          # after a resubscribe the first message again
    assert L.navgpu_costmap3d_destroy(h) == 0


def test_ignored_sequences_without_a_device(nav):
    """the part of the state machine no device is needed for, in full on any machine"""
    L = nav.lib()
    h = make(nav)

    def feed(seqs, instance=0):
        m = messages(1, instance=instance, update_seq=seqs[0], bounds_seq=seqs[1], universe=1)
        out = np.full(1, 77, np.int32)
        assert L.navgpu_costmap3d_layer_update_cells(h, 1, vp(m), vp(u32(1)), AS_GIVEN, None, 0, None, 0, vp(out)) == 0
        return int(out[0])

    for _ in range(3):
        assert feed((5, 5)) == IGNORED and feed((5, 4)) == RESYNC
    assert feed((0, 0)) == IGNORED and L.navgpu_costmap3d_layer_resubscribe(h, 0, 1) == 0 and feed((0, 0)) == IGNORED
    assert feed((0xFFFFFFFF, 0xFFFFFFFF), instance=2) == IGNORED and feed((0, 0xFFFFFFFF), instance=2) == RESYNC
    # configure_layers resets every pair's state
    from navigation_amd import _lib
    recs = (_lib.C3dLayer * len(STACK))()
    for k, s in enumerate(STACK):
        recs[k] = _lib.C3dLayer(**dict(dict(enabled=1, combination_method=1, max_cloud_points=8), **s))
    assert feed((1, 1), instance=1) == IGNORED
    assert L.navgpu_costmap3d_configure_layers(h, recs, len(STACK), 127) == 0
    assert feed((1, 1), instance=1) == IGNORED               # (RESYNC if the state had survived)
    assert L.navgpu_costmap3d_destroy(h) == 0


def test_a_handle_that_never_configures_the_publisher_behaves_as_before(nav):
    from navigation_amd import costmap3d
    L = nav.lib()
    h = make(nav)
    one, poses, out = u32(0), np.zeros((2, 3)), np.zeros((2, 4))
    cloud = np.zeros(1, costmap3d.CLOUD_DTYPE)
    cloud[0] = (0, 1, 0, 1, costmap3d.IDENTITY_TRANSFORM)
    pts = np.zeros((1, 3), np.float32)
    assert L.navgpu_costmap3d_update(h, 2, vp(u32(1, 1)), vp(poses), vp(out)) == INVALID
    assert L.navgpu_costmap3d_update(h, 0, vp(one), vp(poses), vp(out)) == 0
    assert L.navgpu_costmap3d_reset(h, 2, vp(u32(0, 1))) == 0
    assert L.navgpu_costmap3d_buffer_clouds(h, vp(cloud), 1, vp(np.zeros((2, 3), np.float32)), 2, None) == CAPACITY   # max_cloud_points = 1: the fed layer's
    assert L.navgpu_costmap3d_buffer_clouds(h, vp(cloud), 0, vp(pts), 1, None) == 0
    assert L.navgpu_costmap3d_roll(h, 1, vp(one), 1, vp(ALIGNED[:2].copy()), None) == 0
    if L.navgpu_device_count() <= 0:
        assert L.navgpu_costmap3d_buffer_clouds(h, vp(cloud), 1, vp(pts), 1, None) == NO_DEVICE
        assert L.navgpu_costmap3d_update(h, 1, vp(one), vp(poses), vp(out)) == NO_DEVICE
    assert L.navgpu_costmap3d_destroy(h) == 0
