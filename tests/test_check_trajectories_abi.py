"""CPU-side checks of the batched checkTrajectory entry point (navgpu_planner_check_trajectories): it is declared, exported and bound,
its kernel id and the kernel count agree between include/navgpu.h (as the C compiler sees it) and the Python tables, and the kernel
has its name in the profile tables.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_entry_point_is_declared_exported_and_bound(nav):
    from navigation_amd import _lib
    L = nav.lib()
    header = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    name = "navgpu_planner_check_trajectories"
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, "not declared in navgpu.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(args) == 7, args  # fleet, n_robots, instances, probe_offsets, vel_samples, ok, costs
    assert hasattr(L, name)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert name in bound and len(bound[name]) == 7
    assert callable(nav.Fleet.check_trajectories)
    # the single call keeps its signature
    assert re.search(r"\bint navgpu_planner_check_trajectory\(navgpu_fleet\* fleet, uint32_t instance, const float vel_samples\[3\], int32_t\* ok\);", header)
    assert len(bound["navgpu_planner_check_trajectory"]) == 4


def test_kernel_id_and_count_match_header(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "ids.c"  # as C: the header is a C header
    src.write_text('#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("kernel %d %d\\n", NAVGPU_K_CHECK_TRAJ, NAVGPU_K_COUNT);return 0;}\n')
    exe = tmp_path / "ids"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert out.strip() == f"kernel {_lib.K_CHECK_TRAJ} {len(_lib.KERNELS)}"
    assert _lib.K_CHECK_TRAJ == 9 and len(_lib.KERNELS) == 10


def test_kernel_name(nav):
    from navigation_amd import _lib
    L = nav.lib()
    assert L.navgpu_kernel_name(9) == b"k_check_traj"
    assert _lib.KERNELS[_lib.K_CHECK_TRAJ] == "k_check_traj"
    for k, name in enumerate(_lib.KERNELS):  # the ids before it have not moved
        assert L.navgpu_kernel_name(k) == name.encode()


def test_argument_errors_need_no_gpu(nav):
    """argument checks come before anything touches a device"""
    L = nav.lib()
    assert L.navgpu_planner_check_trajectories(None, 1, None, None, None, None, None) == -1
