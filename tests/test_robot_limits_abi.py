"""navgpu_robot_limits / navgpu_planner_set_limits / _get_limits without a GPU: the struct's layout as the C compiler sees navgpu.h
against the ctypes mirror, the symbols, and Fleet.set_limits' own checks (a malformed record never reaches the library)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()
    return nav


def test_struct_layout_matches_header(nav, tmp_path):
    from navigation_amd import _lib
    names = [n for n, _ in _lib.RobotLimits._fields_]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "navgpu.h"\nint main(){printf("%zu", sizeof(navgpu_robot_limits));\n' +
                   "".join(f'printf(" %zu", offsetof(navgpu_robot_limits, {n}));\n' for n in names) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.RobotLimits) == 15 * 8 + 8
    assert out[1:] == [getattr(_lib.RobotLimits, n).offset for n in names]
    # the eleven leading fields are navgpu_dwa_config's, in its order: one record feeds the planner as a configuration does
    assert names[:11] == [n for n, _ in _lib.DwaConfig._fields_[:11]]
    assert [getattr(_lib.RobotLimits, n).offset for n in names[:11]] == [getattr(_lib.DwaConfig, n).offset for n in names[:11]]


def test_symbols_exported_and_bound(nav):
    L = nav.lib()
    for name in ("navgpu_planner_set_limits", "navgpu_planner_get_limits"):
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 4
    assert L.navgpu_planner_set_limits(None, 0, 1, None) == -1  # NAVGPU_ERR_INVALID before anything is touched
    assert L.navgpu_planner_get_limits(None, 0, 1, None) == -1


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


GOOD = dict(max_trans_vel=0.25, min_trans_vel=0.1, max_vel_x=0.55, min_vel_x=0.0, max_vel_y=0.1, min_vel_y=-0.1, max_rot_vel=0.45, min_rot_vel=0.4,
            acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2, xy_goal_tolerance=0.1, yaw_goal_tolerance=0.05, trans_stopped_vel=0.1,
            rot_stopped_vel=0.1, prune_plan=1)


def test_set_limits_rejects_a_malformed_record_before_any_library_call(nav):
    fl = object.__new__(nav.Fleet)
    fl.L, fl.h, fl.n = _NoLibrary(), None, 4
    missing = {k: v for k, v in GOOD.items() if k != "acc_lim_y"}
    for bad in ([missing], [GOOD, dict(GOOD, max_speed=1.0)], [dict(GOOD, max_rot_vel="fast")], [dict(GOOD, max_vel_x=None)], [], [0.25],
                np.zeros((2, 16)), [dict(GOOD, min_vel_x=True)]):
        with pytest.raises(ValueError):
            fl.set_limits(bad)
    # what a well-formed list, dict or structured array becomes
    rec = nav.Fleet._limit_records([GOOD, dict(GOOD, prune_plan=0)])
    assert len(rec) == 2 and rec[0].as_dict() == GOOD and rec[1].prune_plan == 0 and rec[0].reserved == 0
    assert nav.Fleet._limit_records(GOOD)[0].as_dict() == GOOD
    arr = np.zeros(2, [(k, np.int32 if k == "prune_plan" else np.float64) for k in GOOD])
    for k, v in GOOD.items():
        arr[k] = v
    rec = nav.Fleet._limit_records(arr)
    assert len(rec) == 2 and rec[1].as_dict() == GOOD
    with pytest.raises(AssertionError):  # and only a well-formed one goes on to the library
        fl.set_limits([GOOD])
    fl.h = None  # (nothing to destroy)
