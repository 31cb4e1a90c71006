"""CPU-side checks of the planner cycle for a robot list (navgpu_planner_stage_list, _stage_poses_list, _cycle_list, _results_list):
declared, exported and bound; no new kernel id, as the C compiler sees include/navgpu.h; argument errors that need no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {"navgpu_planner_stage_list": 6, "navgpu_planner_stage_poses_list": 5, "navgpu_planner_cycle_list": 3, "navgpu_planner_results_list": 4}
METHODS = ("stage_planner_list", "stage_poses_list", "planner_cycle_list", "results_list")


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
    assert [len(bound["navgpu_planner_" + n]) for n in ("stage", "stage_poses", "cycle", "results")] == [6, 5, 3, 4]


def test_no_new_kernel_id(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "kcount.c"  # as C: the header is a C header
    src.write_text('#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("%d\\n", NAVGPU_K_COUNT);return 0;}\n')
    exe = tmp_path / "kcount"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    k_count = int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    assert k_count == 10 == len(_lib.KERNELS)  # the listed launches are timed under k_bfs, k_score and k_select


def test_argument_errors_need_no_gpu(nav):
    """argument checks come before anything touches a device"""
    L = nav.lib()
    inst = np.asarray([0, 2], np.uint32)
    p = inst.ctypes.data_as(C.c_void_p)
    buf = np.zeros(64)
    q = buf.ctypes.data_as(C.c_void_p)
    assert L.navgpu_planner_stage_list(None, 2, p, q, q, 2) == -1
    assert L.navgpu_planner_stage_poses_list(None, 2, p, q, q) == -1
    assert L.navgpu_planner_cycle_list(None, 2, p) == -1
    assert L.navgpu_planner_results_list(None, 2, p, q) == -1
