"""CPU-side checks of the legacy planner's listed entry points (navgpu_tp_update_plans_list, navgpu_tp_find_best_path_list): declared,
exported and bound; argument errors that need no device; the kernel-id count as the C compiler sees include/navgpu.h.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {"navgpu_tp_update_plans_list": 6, "navgpu_tp_find_best_path_list": 5}
METHODS = ("tp_update_plans_list", "tp_find_best_path_list")


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
    # the range calls keep their signatures
    assert len(bound["navgpu_tp_update_plans"]) == 6 and len(bound["navgpu_tp_find_best_path"]) == 5


def test_null_fleet_is_invalid(nav):
    """argument checks come before anything touches a device"""
    L = nav.lib()
    inst, off = np.asarray((0, 2), np.uint32), np.asarray((0, 0, 0), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.navgpu_tp_update_plans_list(None, 2, p(inst), None, p(off), 0) == -1
    assert L.navgpu_tp_update_plans_list(None, 0, None, None, p(off), 1) == -1
    assert L.navgpu_tp_find_best_path_list(None, 2, p(inst), None, None) == -1
    assert L.navgpu_tp_find_best_path_list(None, 0, None, None, None) == -1


def test_kernel_count_is_still_ten(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "tplist.c"  # as C: the header is a C header
    src.write_text('#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("%d %d %d\\n", NAVGPU_K_COUNT, NAVGPU_K_BFS, NAVGPU_K_SCORE);return 0;}\n')
    exe = tmp_path / "tplist"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    k_count, k_bfs, k_score = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert k_count == 10 == len(_lib.KERNELS)  # the listed launches are timed under k_bfs and k_score: no new kernel id
    assert _lib.KERNELS[k_bfs] == "k_bfs" and _lib.KERNELS[k_score] == "k_score"
