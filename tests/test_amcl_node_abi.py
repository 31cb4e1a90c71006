"""CPU checks of the amcl node C-ABI (navgpu_amcl_node_*, navgpu_amcl_hypotheses): the entry points are declared, exported and
bound, the four structs agree with include/navgpu.h field by field, and null handles / arguments are rejected before any device
work.  That a refused configuration leaves the previous one in force needs a handle, hence a device: that test is marked gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"navgpu_amcl_node_configure": 2, "navgpu_amcl_node_laser_received": 7, "navgpu_amcl_hypotheses": 4, "navgpu_amcl_node_reset": 4,
       "navgpu_amcl_node_request_nomotion_update": 3, "navgpu_amcl_node_integrate_odom": 4, "navgpu_amcl_node_get_state": 4,
       "navgpu_amcl_node_set_state": 4}
METHODS = ["configure_node", "laser_received", "hypotheses", "node_reset", "request_nomotion_update", "integrate_odom", "node_state",
           "set_node_state"]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_node_entry_points_are_declared_exported_and_bound(nav):
    from navigation_amd import _lib
    from navigation_amd.localization import AmclLaser
    src = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    L = nav.lib()
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert name in bound and len(bound[name][1]) == nargs, name
    for m in METHODS:
        assert callable(getattr(AmclLaser, m)), m
    assert len(_lib.KERNELS) == 10  # the amcl handle's kernels carry no kernel id


def flat_fields(struct):
    """(name, offset, size) of every field of a ctypes Structure"""
    return [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_]


@pytest.mark.parametrize("cname, pyname", [("navgpu_amcl_node_params", "AmclNodeParams"), ("navgpu_amcl_scan", "AmclScan"),
                                           ("navgpu_amcl_node_result", "AmclNodeResult"), ("navgpu_amcl_node_state", "AmclNodeState")])
def test_struct_layouts_agree_with_the_header(nav, tmp_path, cname, pyname):
    from navigation_amd import _lib
    S = getattr(_lib, pyname)
    fields = flat_fields(S)
    hdr = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"\[\d+\]", "", d.strip()) for stmt in body.split(";") if stmt.strip()
                for d in stmt.strip().split(None, 1)[1].split(",")]
    assert declared == [n for n, _, _ in fields]  # the same fields in the same order, none missing on either side
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "navgpu.h"\nint main(){%s x;printf("%%zu' % cname +
                   " %zu %zu" * len(fields) + '\\n", sizeof(x),' +
                   ",".join(f"offsetof({cname}, {n}), sizeof(x.{n})" for n, _, _ in fields) + ');return 0;}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert v[0] == C.sizeof(S)
    assert list(zip(v[1::2], v[2::2])) == [(o, s) for _, o, s in fields]
    # the numpy views the Python layer hands out are the same bytes
    assert np.dtype(S).itemsize == C.sizeof(S)


def test_null_handle_and_arguments_are_invalid(nav):
    from navigation_amd import _lib
    L = nav.lib()
    p = _lib.AmclNodeParams()
    scans = (_lib.AmclScan * 2)()
    res = (_lib.AmclNodeResult * 2)()
    st = (_lib.AmclNodeState * 2)()
    raw = (C.c_float * 8)()
    poses = (C.c_double * 6)()
    assert L.navgpu_amcl_node_configure(None, C.byref(p)) == -1
    assert L.navgpu_amcl_node_laser_received(None, 0, 2, scans, raw, 0, res) == -1
    assert L.navgpu_amcl_hypotheses(None, 0, 2, res) == -1
    assert L.navgpu_amcl_node_reset(None, 0, 2, 0) == -1
    assert L.navgpu_amcl_node_request_nomotion_update(None, 0, 2) == -1
    assert L.navgpu_amcl_node_integrate_odom(None, 0, 2, poses) == -1
    assert L.navgpu_amcl_node_get_state(None, 0, 2, st) == -1
    assert L.navgpu_amcl_node_set_state(None, 0, 2, st) == -1


@pytest.mark.gpu
def test_null_arguments_and_bad_parameters_on_a_handle(nav):
    from navigation_amd import _lib
    if nav.lib().navgpu_device_count() <= 0:
        pytest.skip("no GPU")
    L = nav.lib()
    a = nav.AmclLaser(2, 16, max_beams=8)
    res = (_lib.AmclNodeResult * 2)()
    scans = (_lib.AmclScan * 2)()
    st = (_lib.AmclNodeState * 2)()
    assert L.navgpu_amcl_node_configure(a.h, None) == -1
    assert L.navgpu_amcl_node_laser_received(a.h, 0, 2, None, None, 0, res) == -1
    assert L.navgpu_amcl_node_laser_received(a.h, 0, 2, scans, None, 0, None) == -1
    assert L.navgpu_amcl_node_laser_received(a.h, 1, 2, scans, None, 0, res) == -1  # past the last filter
    assert L.navgpu_amcl_hypotheses(a.h, 0, 2, None) == -1
    assert L.navgpu_amcl_node_integrate_odom(a.h, 0, 2, None) == -1
    assert L.navgpu_amcl_node_get_state(a.h, 0, 3, st) == -1
    assert L.navgpu_amcl_node_set_state(a.h, 0, 2, None) == -1
    # configure is all or nothing: a refused struct leaves the configuration in force as it was
    a.configure(max_beams=8)
    a.configure_odom(0)
    a.configure_resample(min_samples=4)
    a.set_map(np.zeros((8, 8), np.int8), 0.1)
    a.set_samples(np.zeros((2, 16, 3)), np.full((2, 16), 1 / 16))
    a.configure_node(d_thresh=0.5, a_thresh=0.5, resample_interval=3)
    for bad in (dict(resample_interval=0), dict(resample_interval=-2), dict(d_thresh=float("nan")), dict(a_thresh=float("nan")),
                dict(laser_max_range=float("nan")), dict(use_odom_integrator=2)):
        p = _lib.AmclNodeParams(d_thresh=0.0, a_thresh=0.0, resample_interval=1)
        for k, v in bad.items():
            setattr(p, k, v)
        assert L.navgpu_amcl_node_configure(a.h, C.byref(p)) == -1, bad
    scan = dict(ranges=np.full(8, 0.3, np.float32), range_min=0.05, range_max=5.0, yaw_min=-0.5, yaw_inc=-0.4, odom_pose=(0.0, 0.0, 0.0))
    a.laser_received([scan, scan])             # the first scan
    for i in (1, 2, 3):                        # 0.3 m per scan: below the d_thresh 0.5 still in force, and interval 3 holds
        scan["odom_pose"] = (0.3 * i, 0.0, 0.0)
        _, r = a.laser_received([scan, None])
        assert r.moved[0] == (1 if i == 2 else 0), i   # 0.3 no; 0.6 since the last update yes; then 0.3 again no
        assert r.resampled[0] == 0
    assert a.node_state().resample_count[0] == 2
    a.close()
