"""CPU-side checks of the layered costmap_3d update's C-ABI (include/navgpu_costmap3d_layers.h, included by navgpu.h): the ctypes
mirrors and numpy records agree with the header field by field as the C compiler sees it, so do the constants; the entry points are
declared, exported and bound and each cites the reference lines it replaces; every argument error is found on the host, before a
device is opened - so all of this gives the same answers on a machine without one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("navgpu_costmap3d_configure_layers", "navgpu_costmap3d_layer_set", "navgpu_costmap3d_buffer_clouds", "navgpu_costmap3d_set_static_grid",
                "navgpu_costmap3d_update", "navgpu_costmap3d_reset", "navgpu_costmap3d_layer2d_download", "navgpu_costmap3d_layer2d_update_costs",
                "navgpu_costmap3d_layer_columns_download", "navgpu_costmap3d_free_columns_download")
INVALID, NO_DEVICE, CAPACITY, STATE = -1, -2, -4, -5


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_struct_layout_matches_header(tmp_path):
    from navigation_amd import _lib, costmap3d
    structs = {"navgpu_c3d_layer": (_lib.C3dLayer, None, 56), "navgpu_c3d_cloud": (_lib.C3dCloud, costmap3d.CLOUD_DTYPE, 112)}
    constants = {"NAVGPU_C3D_MAX_LAYERS": _lib.C3D_MAX_LAYERS, "NAVGPU_C3D_LAYER_POINT_CLOUD": _lib.C3D_LAYER_POINT_CLOUD,
                 "NAVGPU_C3D_LAYER_STATIC_2D": _lib.C3D_LAYER_STATIC_2D, "NAVGPU_C3D_LAYER_CYLINDER_CLEARING": _lib.C3D_LAYER_CYLINDER_CLEARING,
                 "NAVGPU_C3D_COMBINE_OVERWRITE": _lib.C3D_COMBINE_OVERWRITE, "NAVGPU_C3D_COMBINE_MAXIMUM": _lib.C3D_COMBINE_MAXIMUM,
                 "NAVGPU_C3D_COMBINE_IF_UNKNOWN": _lib.C3D_COMBINE_IF_UNKNOWN, "NAVGPU_C3D_COMBINE_NOTHING": _lib.C3D_COMBINE_NOTHING}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "navgpu.h"', 'int main(){']
    for name, (mirror, _, _) in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    for name in constants:
        lines.append(f'printf("{name} %d\\n", (int){name});')
    lines.append('return 0;}')
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, (mirror, dtype, size) in structs.items():
        assert int(out[name]) == C.sizeof(mirror) == size, name
        for field, _ in mirror._fields_:
            assert int(out[f"{name}.{field}"]) == getattr(mirror, field).offset, (name, field)
            if dtype is not None:
                assert dtype.fields[field][1] == getattr(mirror, field).offset, (name, field)
        if dtype is not None:
            assert dtype.itemsize == size and tuple(dtype.names) == tuple(f for f, _ in mirror._fields_)
    for name, value in constants.items():
        assert int(out[name]) == value, name
    # costmap_3d/cfg/GenericPlugin.cfg's numbers
    assert (_lib.C3D_COMBINE_OVERWRITE, _lib.C3D_COMBINE_MAXIMUM, _lib.C3D_COMBINE_IF_UNKNOWN, _lib.C3D_COMBINE_NOTHING) == (0, 1, 2, 99)


def test_entry_points_are_declared_exported_bound_and_cite_the_reference(nav):
    from navigation_amd import _lib
    L = nav.lib()
    assert '#include "navgpu_costmap3d_layers.h"' in open(os.path.join(ROOT, "include", "navgpu.h")).read()
    header = open(os.path.join(ROOT, "include", "navgpu_costmap3d_layers.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ENTRY_POINTS:
        m = re.search(r"\bint " + name + r"\(", header)
        assert m, name
        assert hasattr(L, name) and name in bound, name
        comment = header[header.rindex("/*", 0, m.start()):header.rindex("*/", 0, m.start())]
        assert re.search(r"\w+\.(cpp|h):\d+(-\d+)?", comment), name
    assert set(re.findall(r"\bint (navgpu_costmap3d_\w+)\(", header)) == set(ENTRY_POINTS)
    for method in ("configure_layers", "layer_set", "buffer_clouds", "set_static_grid", "update", "reset", "layer2d", "update_costs_2d", "layer_columns",
                   "free_columns"):
        assert callable(getattr(nav.Costmap3D, method))


def make(nav, **kw):
    from navigation_amd import _lib
    d = dict(n_instances=2, size_x=16, size_y=8, size_z=64, resolution=0.25, max_triangles=4, max_boxes=4, max_poses=4, device=0)
    d.update(kw)
    h = C.c_void_p()
    assert nav.lib().navgpu_costmap3d_create(C.byref(_lib.Costmap3DDesc(**d)), C.byref(h)) == 0
    return h


def layer_records(*specs):
    from navigation_amd import _lib
    recs = (_lib.C3dLayer * max(len(specs), 1))()
    for k, s in enumerate(specs):
        d = dict(enabled=1, combination_method=1, max_cloud_points=8)
        d.update(s)
        recs[k] = _lib.C3dLayer(**d)
    return recs


STACK = (dict(kind=1, height=0.0, lethal_cost_threshold=100), dict(kind=0), dict(kind=2, radius=-0.5))


def test_null_handles(nav):
    L = nav.lib()
    p = vp(np.zeros(16))
    assert L.navgpu_costmap3d_configure_layers(None, p, 1, 127) == INVALID
    assert L.navgpu_costmap3d_layer_set(None, 0, 1, 1) == INVALID
    assert L.navgpu_costmap3d_buffer_clouds(None, p, 0, p, 0, None) == INVALID
    assert L.navgpu_costmap3d_set_static_grid(None, 0, 0, p, 1, 1, 0.0, 0.0, None) == INVALID
    assert L.navgpu_costmap3d_update(None, 0, p, p, p) == INVALID
    assert L.navgpu_costmap3d_reset(None, 0, p) == INVALID
    assert L.navgpu_costmap3d_layer2d_download(None, 0, 0, 0, 1, 1, p) == INVALID
    assert L.navgpu_costmap3d_layer2d_update_costs(None, 0, p, p, 0, 0, 0, 0, p, 0) == INVALID
    assert L.navgpu_costmap3d_layer_columns_download(None, 0, 0, None, None, None, None) == INVALID
    assert L.navgpu_costmap3d_free_columns_download(None, 0, None) == INVALID


def test_layer_calls_before_configure_are_a_state_error(nav):
    L = nav.lib()
    h = make(nav)
    one = np.zeros(1, np.uint32)
    pose, out = np.zeros(3), np.zeros(4)
    cloud = np.zeros(1, nav.costmap3d.CLOUD_DTYPE)
    pts = np.zeros((1, 3), np.float32)
    grid = np.zeros((1, 1), np.int8)
    assert L.navgpu_costmap3d_layer_set(h, 0, 1, 1) == STATE
    assert L.navgpu_costmap3d_buffer_clouds(h, vp(cloud), 1, vp(pts), 1, None) == STATE
    assert L.navgpu_costmap3d_set_static_grid(h, 0, 0, vp(grid), 1, 1, 0.0, 0.0, None) == STATE
    assert L.navgpu_costmap3d_update(h, 1, vp(one), vp(pose), vp(out)) == STATE
    assert L.navgpu_costmap3d_reset(h, 1, vp(one)) == STATE
    assert L.navgpu_costmap3d_layer2d_download(h, 0, 0, 0, 1, 1, vp(np.zeros(1, np.uint8))) == STATE
    assert L.navgpu_costmap3d_layer2d_update_costs(h, 1, vp(one), vp(pose), 128, 2, 16, 8, vp(np.zeros(4, np.int32)), 1) == STATE
    assert L.navgpu_costmap3d_layer_columns_download(h, 0, 0, None, None, None, None) == STATE
    assert L.navgpu_costmap3d_free_columns_download(h, 0, None) == STATE
    assert L.navgpu_costmap3d_destroy(h) == 0


def test_configure_checks_the_layers(nav):
    L = nav.lib()
    h = make(nav)
    conf = lambda recs, n, nl=127: L.navgpu_costmap3d_configure_layers(h, recs, n, nl)
    assert conf(layer_records(*STACK), 0) == INVALID
    assert conf(layer_records(*([STACK[1]] * 9)), 9) == INVALID                                         # more than 8 layers
    assert conf(layer_records(dict(kind=3)), 1) == INVALID                                              # kind
    assert conf(layer_records(dict(kind=-1)), 1) == INVALID
    assert conf(layer_records(dict(kind=0, combination_method=3)), 1) == INVALID                        # GenericPlugin.cfg has 0, 1, 2, 99
    assert conf(layer_records(dict(kind=0, max_cloud_points=0)), 1) == INVALID
    assert conf(layer_records(dict(kind=0, cloud_has_intensity=1, free_intensity=1.0, lethal_intensity=1.0)), 1) == INVALID
    assert conf(layer_records(dict(kind=0, cloud_has_intensity=1, free_intensity=float("nan"), lethal_intensity=1.0)), 1) == INVALID
    assert conf(layer_records(dict(kind=1, lethal_cost_threshold=256)), 1) == INVALID
    assert conf(layer_records(dict(kind=1, height=float("inf"))), 1) == INVALID
    assert conf(layer_records(dict(kind=2, radius=float("nan"))), 1) == INVALID
    assert conf(layer_records(*STACK), 3, 256) == INVALID and conf(layer_records(*STACK), 3, -1) == INVALID
    assert conf(layer_records(*STACK), 3) == 0                                                          # host state until a call needs the device
    assert conf(layer_records(*([STACK[1]] * 8)), 8) == 0                                               # a second call reconfigures
    assert L.navgpu_costmap3d_destroy(h) == 0


def test_argument_errors_need_no_gpu(nav):
    from navigation_amd import costmap3d
    L = nav.lib()
    h = make(nav)
    assert L.navgpu_costmap3d_configure_layers(h, layer_records(*STACK), 3, 127) == 0
    aligned = np.array([-2.0, 1.0, -0.5])
    for i in (0, 1):
        assert L.navgpu_costmap3d_set_origin(h, i, vp(aligned)) == 0
    pts = np.zeros((8, 3), np.float32)

    def clouds(*rows):
        c = np.zeros(len(rows), costmap3d.CLOUD_DTYPE)
        for k, r in enumerate(rows):
            c[k] = tuple(r) + (costmap3d.IDENTITY_TRANSFORM,)
        return c

    def buffer(c, n_points=8):
        return L.navgpu_costmap3d_buffer_clouds(h, vp(c), len(c), vp(pts), n_points, None)

    assert buffer(clouds((0, 1, 0, 4), (0, 1, 4, 4))) == INVALID                                        # two clouds for one (instance, layer)
    assert buffer(clouds((0, 1, 0, 4), (1, 1, 4, 5))) == INVALID                                        # ends beyond n_points
    assert buffer(clouds((2, 1, 0, 4))) == INVALID                                                      # instance
    assert buffer(clouds((0, 3, 0, 4))) == INVALID                                                      # layer index
    assert buffer(clouds((0, 0, 0, 4))) == INVALID and buffer(clouds((0, 2, 0, 4))) == INVALID          # not a POINT_CLOUD layer
    big = np.zeros((9, 3), np.float32)
    assert L.navgpu_costmap3d_buffer_clouds(h, vp(clouds((0, 1, 0, 4))), 1, vp(big), 9, None) == CAPACITY  # max_cloud_points is 8
    bad_tf = clouds((0, 1, 0, 4))
    bad_tf["transform"][0, 3] = np.nan
    assert buffer(bad_tf) == INVALID

    grid = np.zeros((8, 16), np.int8)
    static = lambda inst=0, layer=0, w=16, hh=8, ox=-2.0, oy=1.0: L.navgpu_costmap3d_set_static_grid(h, inst, layer, vp(grid), w, hh, ox, oy, None)
    assert static(layer=1) == INVALID and static(layer=2) == INVALID and static(layer=3) == INVALID     # not a STATIC_2D layer
    assert static(inst=2) == INVALID and static(w=0) == INVALID and static(hh=0) == INVALID and static(ox=float("nan")) == INVALID
    assert static(w=1 << 14, hh=(1 << 12) + 1) == INVALID

    one, two = np.array([0], np.uint32), np.array([1, 1], np.uint32)
    poses, out = np.zeros((2, 3)), np.zeros((2, 4))
    assert L.navgpu_costmap3d_update(h, 2, vp(two), vp(poses), vp(out)) == INVALID                      # listed twice
    assert L.navgpu_costmap3d_update(h, 1, vp(np.array([2], np.uint32)), vp(poses), vp(out)) == INVALID
    assert L.navgpu_costmap3d_update(h, 1, vp(one), vp(np.array([0.0, np.nan, 0.0])), vp(out)) == INVALID
    assert L.navgpu_costmap3d_reset(h, 1, vp(np.array([2], np.uint32))) == INVALID
    assert L.navgpu_costmap3d_reset(h, 2, vp(np.array([0, 1], np.uint32))) == 0                         # host state only so far

    assert L.navgpu_costmap3d_layer_set(h, 3, 1, 1) == INVALID and L.navgpu_costmap3d_layer_set(h, 1, 1, 5) == INVALID
    assert L.navgpu_costmap3d_layer_set(h, 1, 0, 99) == 0 and L.navgpu_costmap3d_layer_set(h, 2, 0, 1) == 0

    byte = np.zeros(16 * 8, np.uint8)
    assert L.navgpu_costmap3d_layer2d_download(h, 2, 0, 0, 1, 1, vp(byte)) == INVALID
    assert L.navgpu_costmap3d_layer2d_download(h, 0, 0, 0, 17, 8, vp(byte)) == INVALID
    assert L.navgpu_costmap3d_layer2d_download(h, 0, 4, 0, 4, 8, vp(byte)) == INVALID
    box = np.array([0, 0, 16, 8], np.int32)
    costs = lambda sx=16, sy=8, b=box, gi=2, ins=one, stride=128: L.navgpu_costmap3d_layer2d_update_costs(h, len(ins), vp(ins), vp(byte), stride, gi, sx, sy, vp(b), 1)
    assert costs(sx=15) == INVALID and costs(sy=9) == INVALID                                           # grid sizes that differ
    assert costs(stride=127) == INVALID
    assert costs(gi=0) == INVALID
    assert costs(b=np.array([0, 0, 17, 8], np.int32)) == INVALID and costs(b=np.array([-1, 0, 16, 8], np.int32)) == INVALID
    assert costs(b=np.array([4, 0, 3, 8], np.int32)) == INVALID
    assert L.navgpu_costmap3d_layer_columns_download(h, 0, 2, None, None, None, None) == INVALID        # a cylinder layer has no planes
    assert L.navgpu_costmap3d_layer_columns_download(h, 2, 0, None, None, None, None) == INVALID
    assert L.navgpu_costmap3d_free_columns_download(h, 2, None) == INVALID

    # an unaligned origin: every layer call that places cells refuses it
    assert L.navgpu_costmap3d_set_origin(h, 0, vp(np.array([-2.0, 1.1, -0.5]))) == 0
    assert buffer(clouds((0, 1, 0, 4))) == INVALID
    assert static() == INVALID
    assert L.navgpu_costmap3d_update(h, 1, vp(one), vp(poses), vp(out)) == INVALID
    assert L.navgpu_costmap3d_set_origin(h, 0, vp(aligned)) == 0
    if L.navgpu_device_count() <= 0:  # and what is valid needs the device: there is no CPU fallback
        assert buffer(clouds((0, 1, 0, 4))) == NO_DEVICE
        assert static() == NO_DEVICE
        assert L.navgpu_costmap3d_update(h, 1, vp(one), vp(poses), vp(out)) == NO_DEVICE
    assert L.navgpu_costmap3d_destroy(h) == 0
