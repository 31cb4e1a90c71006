"""CPU checks of the amcl init C-ABI: the new entry points are declared, exported and bound, navgpu_amcl_uniform_params' layout
agrees with include/navgpu.h, and null handles / arguments are rejected before any device work."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["navgpu_amcl_init_gaussian", "navgpu_amcl_init_uniform"]


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_init_entry_points_are_declared_exported_and_bound(nav):
    from navigation_amd import _lib
    src = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    L = nav.lib()
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert name in bound, name
    assert len(bound["navgpu_amcl_init_gaussian"][1]) == 9
    assert len(bound["navgpu_amcl_init_uniform"][1]) == 12
    from navigation_amd.localization import AmclLaser
    assert callable(AmclLaser.init_gaussian) and callable(AmclLaser.init_uniform)


def test_uniform_params_layout(nav, tmp_path):
    from navigation_amd import _lib
    fields = ["starting_weight_threshold", "deweight_multiplier", "max_candidates"]
    src = tmp_path / "up.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("%zu' + " %zu" * len(fields) +
                   '\\n", sizeof(navgpu_amcl_uniform_params),' + ",".join(f"offsetof(navgpu_amcl_uniform_params, {f})" for f in fields) +
                   ');return 0;}\n')
    exe = tmp_path / "up"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.AmclUniformParams
    assert v[0] == C.sizeof(P) == 24
    assert v[1:] == [getattr(P, f).offset for f in fields] == [0, 8, 16]


def test_null_handle_and_arguments_are_invalid(nav):
    from navigation_amd import _lib
    L = nav.lib()
    st = (C.c_int32 * 2)()
    mean = (C.c_double * 6)()
    cov = (C.c_double * 18)()
    x = (C.c_uint64 * 2)()
    p = _lib.AmclUniformParams(starting_weight_threshold=0.0, deweight_multiplier=0.0, max_candidates=0)
    assert L.navgpu_amcl_init_gaussian(None, 0, 2, mean, cov, _lib.AMCL_DRAW_DRAND48, x, 0, st) == -1
    assert L.navgpu_amcl_init_gaussian(None, 0, 2, None, cov, _lib.AMCL_DRAW_DEVICE, None, 0, st) == -1
    assert L.navgpu_amcl_init_uniform(None, 0, 2, C.byref(p), None, None, None, _lib.AMCL_DRAW_DRAND48, x, 0, None, st) == -1
    assert L.navgpu_amcl_init_uniform(None, 0, 2, None, None, None, None, _lib.AMCL_DRAW_DEVICE, None, 0, None, st) == -1
