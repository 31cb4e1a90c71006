"""CPU-side checks of the footprint-cost / rotate-recovery / carrot-planner part of the C-ABI: the ctypes mirrors of the new structs
agree with include/navgpu.h field by field (sizeof and offsetof as the C compiler sees them), the constants agree, and the new
kernel is in the profile tables."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"navgpu_rotate_recovery_params": "RotateRecoveryParams", "navgpu_rotate_recovery_state": "RotateRecoveryState"}


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
    lines.append('printf("max_sweep %d\\n", NAVGPU_ROTATE_RECOVERY_MAX_SWEEP);')
    lines.append('printf("status %d %d %d\\n", NAVGPU_ROTATE_RUNNING, NAVGPU_ROTATE_DONE, NAVGPU_ROTATE_BLOCKED);')
    lines.append('printf("kernel %d %d\\n", NAVGPU_K_FOOTPRINT, NAVGPU_K_COUNT);')
    lines.append('return 0;}')
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
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
    # every field of the header's structs is mirrored (a field added to the header alone changes sizeof)
    assert f"max_sweep {_lib.ROTATE_RECOVERY_MAX_SWEEP}" in out
    assert f"status {_lib.ROTATE_RUNNING} {_lib.ROTATE_DONE} {_lib.ROTATE_BLOCKED}" in out
    assert f"kernel {_lib.K_FOOTPRINT} {len(_lib.KERNELS)}" in out


def test_defaults_are_the_references():
    from navigation_amd import _lib
    p = _lib.RotateRecoveryParams()  # rotate_recovery.cpp:60-66
    assert (p.sim_granularity, p.acc_lim_th, p.max_rotational_vel, p.min_in_place_rotational_vel, p.yaw_goal_tolerance) == (0.017, 3.2, 1.0, 0.4, 0.10)


def test_new_entry_points_are_exported_and_bound(nav):
    from navigation_amd import _lib
    L = nav.lib()
    header = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("navgpu_footprint_cost", "navgpu_rotate_recovery_configure", "navgpu_rotate_recovery_step", "navgpu_carrot_plan"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(L, name) and name in bound, name
    assert L.navgpu_kernel_name(_lib.K_FOOTPRINT) == b"k_footprint_cost"
    assert _lib.KERNELS[_lib.K_FOOTPRINT] == "k_footprint_cost"


def test_argument_errors_need_no_gpu(nav):
    """argument checks come before anything touches a device"""
    from navigation_amd import _lib
    L = nav.lib()
    assert L.navgpu_footprint_cost(None, 0, 1, None, None, 0, None, None) == -1
    assert L.navgpu_rotate_recovery_configure(None, C.byref(_lib.RotateRecoveryParams())) == -1
    assert L.navgpu_rotate_recovery_step(None, 0, 1, None, None, None, None) == -1
    assert L.navgpu_carrot_plan(None, 0, 1, None, None, 0, None, None) == -1
