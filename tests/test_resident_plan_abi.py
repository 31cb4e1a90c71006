"""Device-resident global plans at the C boundary, without a GPU: the new calls are declared, bound and exported, the ctypes mirror
of navgpu_local_window agrees with the header, every new call names what it replaces, and argument checks come before device work."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["navgpu_local_planner_reserve_plans", "navgpu_local_planner_set_plans", "navgpu_local_planner_adopt_plans",
       "navgpu_local_planner_local_plan", "navgpu_local_planner_windows"]
FIELDS = ["first_index", "n_window", "n_erased", "n_local", "remaining", "status"]


def _header():
    return open(os.path.join(ROOT, "include", "navgpu.h")).read()


def test_local_window_layout_and_constants_match_header(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "sz.c"
    offs = ",".join(f"offsetof(navgpu_local_window,{f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "navgpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n",'
                   'sizeof(navgpu_local_window),' + offs + ',NAVGPU_LOCAL_WINDOW_OK,NAVGPU_LOCAL_WINDOW_NONE,NAVGPU_LOCAL_WINDOW_CAPACITY,'
                   'NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER,NAVGPU_PLAN_FAMILY_NAVFN_ROS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    W = _lib.LocalWindow
    assert [n for n, _ in W._fields_] == FIELDS
    assert v[0] == C.sizeof(W) == 24
    assert v[1:7] == [getattr(W, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20]
    assert v[7:10] == [_lib.LOCAL_WINDOW_OK, _lib.LOCAL_WINDOW_NONE, _lib.LOCAL_WINDOW_CAPACITY] == [0, 1, 2]
    assert v[10:] == [_lib.PLAN_FAMILY_GLOBAL_PLANNER, _lib.PLAN_FAMILY_NAVFN_ROS] == [0, 1]


def test_new_symbols_are_declared_bound_and_exported():
    import navigation_amd as nav
    from navigation_amd import _lib
    if not os.path.exists(nav.lib_path()):
        nav.build()
    L = nav.lib()
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(bound[name][1]), name
        assert hasattr(L, name)
    for name in ("reserve_global_plans", "set_global_plans", "adopt_global_plans", "local_plan", "local_windows", "global_plan"):
        assert callable(getattr(nav.Fleet, name))


def test_every_new_function_names_what_it_replaces():
    hdr = _header()
    cites = {"navgpu_local_planner_reserve_plans": "local_planner_util.cpp", "navgpu_local_planner_set_plans": "dwa_planner_ros.cpp",
             "navgpu_local_planner_adopt_plans": "move_base.cpp", "navgpu_local_planner_local_plan": "dwa_planner_ros.cpp",
             "navgpu_local_planner_windows": "goal_functions.cpp"}
    for name in NEW:
        at = hdr.index("int " + name + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "replaces:" in comment and cites[name] in comment, name


def test_null_and_range_arguments_fail_without_a_device():
    """argument checks come before any device work"""
    import navigation_amd as nav
    L = nav.lib()
    off = (C.c_uint32 * 2)(0, 0)
    assert L.navgpu_local_planner_reserve_plans(None, 16) == -1
    assert L.navgpu_local_planner_set_plans(None, 0, 1, None, off, None) == -1
    assert L.navgpu_local_planner_adopt_plans(None, 0, None, 0, 1, 0, None, None) == -1
    assert L.navgpu_local_planner_local_plan(None, 0, None, 0) == -1
    assert L.navgpu_local_planner_windows(None, 0, 1, None) == -1

