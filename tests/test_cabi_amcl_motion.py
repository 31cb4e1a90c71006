"""CPU checks of the amcl motion-model C-ABI: the new entry points are declared, exported and bound, navgpu_amcl_odom_params'
layout and the new constants agree with include/navgpu.h and with the reference's odom_model_t, and null handles are rejected."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["navgpu_amcl_odom_configure", "navgpu_amcl_update_action"]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_motion_entry_points_are_declared_exported_and_bound(nav):
    from navigation_amd import _lib
    src = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    L = nav.lib()
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert name in bound, name
    from navigation_amd.localization import AmclLaser, drand48_state
    assert callable(AmclLaser.configure_odom) and callable(AmclLaser.update_action)
    assert drand48_state(0) == 0x330E and drand48_state(1) == 0x1330E and drand48_state(-1) == 0xFFFFFFFF330E


def test_odom_params_layout_and_constants(nav, tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "od.c"
    fields = ["model_type", "reserved", "alpha1", "alpha2", "alpha3", "alpha4", "alpha5"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("%zu' + " %zu" * len(fields) +
                   ' %d %d %d %d %d %d %d %d\\n", sizeof(navgpu_amcl_odom_params),' +
                   "".join(f"offsetof(navgpu_amcl_odom_params, {f})," for f in fields) +
                   'NAVGPU_AMCL_ODOM_DIFF, NAVGPU_AMCL_ODOM_OMNI, NAVGPU_AMCL_ODOM_DIFF_CORRECTED, NAVGPU_AMCL_ODOM_OMNI_CORRECTED,'
                   'NAVGPU_AMCL_ODOM_GAUSSIAN, NAVGPU_AMCL_DRAW_SUPPLIED, NAVGPU_AMCL_DRAW_DEVICE, NAVGPU_AMCL_DRAW_DRAND48);return 0;}\n')
    exe = tmp_path / "od"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.AmclOdomParams
    assert v[0] == C.sizeof(P) == 48
    assert v[1:8] == [getattr(P, f).offset for f in fields]
    assert v[8:13] == [_lib.AMCL_ODOM_DIFF, _lib.AMCL_ODOM_OMNI, _lib.AMCL_ODOM_DIFF_CORRECTED, _lib.AMCL_ODOM_OMNI_CORRECTED,
                       _lib.AMCL_ODOM_GAUSSIAN]
    # odom_model_t (amcl_odom.h:38-45): ODOM_MODEL_DIFF, _OMNI, _DIFF_CORRECTED, _OMNI_CORRECTED, _GAUSSIAN in that order
    assert v[8:13] == [0, 1, 2, 3, 4]
    assert v[13:] == [_lib.AMCL_DRAW_SUPPLIED, _lib.AMCL_DRAW_DEVICE, _lib.AMCL_DRAW_DRAND48] == [0, 1, 2]


def test_odom_params_defaults_are_amcl_node(nav):
    from navigation_amd import _lib
    p = _lib.AmclOdomParams()
    assert (p.model_type, p.alpha1, p.alpha2, p.alpha3, p.alpha4, p.alpha5) == (0, 0.2, 0.2, 0.2, 0.2, 0.2)


def test_motion_entry_points_reject_null_handles(nav):
    from navigation_amd import _lib
    L = nav.lib()
    st = (C.c_int32 * 1)()
    odom = (C.c_double * 9)()
    x = (C.c_uint64 * 1)(0x330E)
    assert L.navgpu_amcl_update_action(None, 0, 1, odom, _lib.AMCL_DRAW_DRAND48, x, 0, st) == -1
    assert L.navgpu_amcl_update_action(None, 0, 1, odom, _lib.AMCL_DRAW_DEVICE, None, 0, st) == -1
    p = _lib.AmclOdomParams()
    assert L.navgpu_amcl_odom_configure(None, C.byref(p)) == -1
    assert L.navgpu_amcl_odom_configure(None, None) == -1
