"""CPU-side checks of the observation-buffer part of the C-ABI (navgpu_obsbuf_*): the entry points are declared, exported and
bound, the ctypes mirrors of the three new structs agree with include/navgpu.h field by field (sizeof and offsetof as the C
compiler sees them), the constants agree, and the new kernel is in the profile tables.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"navgpu_obs_source_params": "ObsSourceParams", "navgpu_cloud": "Cloud", "navgpu_obsbuf_robot_status": "ObsBufRobotStatus"}
ENTRY_POINTS = ("navgpu_obsbuf_configure", "navgpu_obsbuf_buffer", "navgpu_obsbuf_stage", "navgpu_obsbuf_observations",
                "navgpu_obsbuf_set_global_frame", "navgpu_obsbuf_reset_last_updated", "navgpu_obsbuf_status")


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_struct_layouts_match_header(tmp_path):
    from navigation_amd import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "navgpu.h"', 'int main(){']
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for field, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'printf("{cname} {field} %zu\\n", offsetof({cname}, {field}));')
    lines.append('printf("kinds %d %d\\n", NAVGPU_CLOUD_XYZ, NAVGPU_CLOUD_SCAN);')
    lines.append('printf("limits %d %d\\n", NAVGPU_OBSBUF_MAX_SOURCES, NAVGPU_OBSBUF_MAX_CLOUD_POINTS);')
    lines.append('printf("kernel %d %d\\n", NAVGPU_K_OBS_INGEST, NAVGPU_K_COUNT);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"  # as C: the header is a C header
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    seen = 0
    for line in out:
        w = line.split()
        if w[0] in STRUCTS:
            cls = getattr(_lib, STRUCTS[w[0]])
            want = C.sizeof(cls) if w[1] == "size" else getattr(cls, w[1]).offset
            assert int(w[2]) == want, line
            seen += 1
    assert seen == sum(1 + len(getattr(_lib, p)._fields_) for p in STRUCTS.values())
    assert f"kinds {_lib.CLOUD_XYZ} {_lib.CLOUD_SCAN}" in out
    assert f"limits {_lib.OBSBUF_MAX_SOURCES} {_lib.OBSBUF_MAX_CLOUD_POINTS}" in out
    assert f"kernel {_lib.K_OBS_INGEST} {len(_lib.KERNELS)}" in out
    # the layout the issue fixes: times are int64 ns, the transform 12 doubles behind the origin
    assert (_lib.Cloud.stamp_ns.offset, _lib.Cloud.origin.offset, _lib.Cloud.transform.offset, C.sizeof(_lib.Cloud)) == (24, 32, 56, 168)
    assert C.sizeof(_lib.ObsSourceParams) == 56


def test_defaults_are_the_references():
    from navigation_amd import _lib
    p = _lib.ObsSourceParams()  # obstacle_layer.cpp:96-140: keep time 0, rate 0, heights 0 .. 2, ranges 2.5 / 3.0, marking + clearing
    assert (p.observation_keep_time_ns, p.expected_update_rate_ns, p.min_obstacle_height, p.max_obstacle_height, p.obstacle_range,
            p.raytrace_range, p.flags, p.inf_is_valid) == (0, 0, 0.0, 2.0, 2.5, 3.0, _lib.OBS_MARKING | _lib.OBS_CLEARING, 0)


def test_entry_points_are_exported_and_bound(nav):
    from navigation_amd import _lib
    L = nav.lib()
    header = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(L, name) and name in bound, name
    assert L.navgpu_kernel_name(_lib.K_OBS_INGEST) == b"k_obs_ingest"
    assert _lib.KERNELS[_lib.K_OBS_INGEST] == "k_obs_ingest"
    for m in ("obs_configure", "obs_buffer", "obs_stage", "obs_observations", "obs_status", "obs_set_global_frame"):
        assert callable(getattr(nav.Fleet, m)), m


def test_argument_errors_need_no_gpu(nav):
    """argument checks come before anything touches a device"""
    from navigation_amd import _lib
    L = nav.lib()
    p = _lib.ObsSourceParams()
    assert L.navgpu_obsbuf_configure(None, C.byref(p), 1, 1, 16) == -1
    assert L.navgpu_obsbuf_buffer(None, None, 0, None, 0, None, 0, 0) == -1
    assert L.navgpu_obsbuf_stage(None, 0, 1, None, 0, None) == -1
    assert L.navgpu_obsbuf_observations(None, 0, 0, None, 0, None, 0, None) == -1
    assert L.navgpu_obsbuf_set_global_frame(None, 0, 1, None) == -1
    assert L.navgpu_obsbuf_reset_last_updated(None, 0, 1, 0) == -1
    assert L.navgpu_obsbuf_status(None, 0, 1, None) == -1


def test_pack_clouds_lays_out_points_and_ranges(nav):
    """Fleet.pack_clouds: `first` runs separately over the packed points and the packed ranges"""
    import numpy as np
    arr, pts, rng = nav.Fleet.pack_clouds([
        dict(instance=2, source=1, stamp_ns=7, points=np.zeros((3, 3), np.float32), origin=(1, 2, 3)),
        dict(instance=0, stamp_ns=8, ranges=np.ones(5, np.float32), angle_min=-1.0, angle_increment=0.5, range_min=0.1, range_max=9.0),
        dict(instance=1, stamp_ns=9, points=np.ones((2, 3), np.float32), transform=range(12))])
    assert [(a.kind, a.first, a.n) for a in arr] == [(0, 0, 3), (1, 0, 5), (0, 3, 2)]
    assert pts.shape == (5, 3) and rng.shape == (5,) and pts.dtype == np.float32
    assert list(arr[0].origin) == [1.0, 2.0, 3.0] and list(arr[0].transform) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert list(arr[2].transform) == list(range(12)) and (arr[1].instance, arr[1].source, arr[1].stamp_ns) == (0, 0, 8)
    assert arr[1].range_max == 9.0 and arr[1].angle_increment == 0.5
