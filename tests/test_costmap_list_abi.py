"""CPU-side checks of the costmap update for a robot list (navgpu_costmap_stage_list, navgpu_obsbuf_stage_list, navgpu_costmap_update_list,
navgpu_costmap_bounds_list): declared, exported and bound; no new kernel id, as the C compiler sees include/navgpu.h; argument errors that
need no device; and that the geometries tests/test_gpu_costmap_list.py uses select the kernels they are meant to select.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {"navgpu_costmap_stage_list": 8, "navgpu_obsbuf_stage_list": 6, "navgpu_costmap_update_list": 3, "navgpu_costmap_bounds_list": 4}
METHODS = ("stage_observations_list", "obs_stage_list", "update_map_list", "bounds_list")

# ---- the geometries of tests/test_gpu_costmap_list.py (imported from here, so that both files speak of the same numbers)
RES = 0.05
N_ROBOTS, ROWS = 12, 80
WIDTH_ALIGNED, WIDTH_UNALIGNED = 96, 130
# inflation radius in metres -> the kernel launch_inflate picks for it (costmap_kernels.hip): k_inflate_bits<11> for R == 11 cells,
# k_inflate_bits<0> for every other R in 1 .. 14, k_inflate beyond; priority_queue_order takes k_inflate_pq whatever R
INFLATION = {"bits11": 0.54, "bits": 0.33, "tile": 0.78}
NINE = (0, 2, 3, 5, 6, 7, 8, 10, 11)


def cell_radius(radius, res=RES):
    """cell_inflation_radius_ = cellDistance(inflation_radius) (inflation_layer.cpp:305, costmap_2d.cpp:181-185), as navgpu_inflation_configure takes it"""
    return int(max(0.0, math.ceil(radius / res)))


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_entry_points_are_declared_exported_and_bound(nav):
    from navigation_amd import _lib
    L = nav.lib()
    header = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    for name, n_args in NAMES.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} not declared in navgpu.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert len(args) == n_args, (name, args)
        assert hasattr(L, name), f"{name} not exported"
        assert name in bound and len(bound[name]) == n_args, name
    for method in METHODS:
        assert callable(getattr(nav.Fleet, method)), method
    # the range forms keep their signatures
    assert [len(bound["navgpu_" + n]) for n in ("costmap_stage", "obsbuf_stage", "costmap_update", "costmap_bounds")] == [8, 6, 3, 4]


def test_no_new_kernel_id(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "kcount.c"  # as C: the header is a C header
    src.write_text('#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("%d\\n", NAVGPU_K_COUNT);return 0;}\n')
    exe = tmp_path / "kcount"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    k_count = int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    assert k_count == 10 == len(_lib.KERNELS)  # the listed launches are timed under k_obstacle, k_merge and k_inflate


def test_argument_errors_need_no_gpu(nav):
    """argument checks come before anything touches a device"""
    L = nav.lib()
    inst = np.asarray([0, 2], np.uint32)
    p = inst.ctypes.data_as(C.c_void_p)
    buf = np.zeros(64)
    q = buf.ctypes.data_as(C.c_void_p)
    assert L.navgpu_costmap_stage_list(None, 2, p, q, None, 0, None, 0) == -1
    assert L.navgpu_obsbuf_stage_list(None, 2, p, q, 0, None) == -1
    assert L.navgpu_costmap_update_list(None, 2, p) == -1
    assert L.navgpu_costmap_bounds_list(None, 2, p, q) == -1
    assert L.navgpu_costmap_stage_list(None, 2, None, q, None, 0, None, 0) == -1
    assert L.navgpu_obsbuf_stage_list(None, 2, None, q, 0, None) == -1
    assert L.navgpu_costmap_update_list(None, 2, None) == -1
    assert L.navgpu_costmap_bounds_list(None, 2, None, q) == -1


def test_geometries_take_the_kernels_named():
    """what launch_inflate and launch_merge branch on, for the shapes of the GPU tests"""
    R = {k: cell_radius(r) for k, r in INFLATION.items()}
    assert R["bits11"] == 11                      # k_inflate_bits<11, .>
    assert 1 <= R["bits"] <= 14 and R["bits"] != 11  # k_inflate_bits<0, .>
    assert 14 < R["tile"] <= 64                   # k_inflate (64 cells: navgpu_inflation_configure's capacity)
    assert WIDTH_ALIGNED % 16 == 0 and WIDTH_UNALIGNED % 16 != 0  # k_merge<ALIGNED = true | false>
    # k_inflate_bits' tiles are 64 columns x 32 rows: three in each direction at the unaligned width, the last ones partial
    assert (-(-WIDTH_UNALIGNED // 64), -(-ROWS // 32)) == (3, 3) and WIDTH_UNALIGNED % 64 and ROWS % 32
    # the nine-entry list: more than one z-slice of eight robots with a partial second one; runs of one, two and four; without the
    # first-but-one and the last-but-two
    assert len(NINE) == 9 and len(NINE) > 8 and len(NINE) % 8
    runs, cur = [], 1
    for a, b in zip(NINE, NINE[1:]):
        if b == a + 1:
            cur += 1
        else:
            runs.append(cur)
            cur = 1
    runs.append(cur)
    assert sorted(set(runs)) == [1, 2, 4] and 1 not in NINE and N_ROBOTS - 3 not in NINE
    assert list(NINE) == sorted(set(NINE)) and NINE[-1] < N_ROBOTS
