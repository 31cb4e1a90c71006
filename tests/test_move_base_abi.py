"""move_base's executive at the C boundary, without a GPU: the new calls are declared, bound and exported, the ctypes mirror of
navgpu_handover_record agrees with the header, every new call names what it replaces, and argument checks come before device work."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["navgpu_costmap_set_polygon_cost", "navgpu_move_base_clear_costmap_windows", "navgpu_move_base_handover_plans",
       "navgpu_move_base_reset_persistence", "navgpu_move_base_get_persistence", "navgpu_move_base_set_persistence",
       "navgpu_move_base_plan_service_candidates", "navgpu_move_base_plan_service", "navgpu_navfn_set_costmap_from_fleet_instance"]
FIELDS = ["decision", "closest_index", "prev_len", "new_len", "dropped", "reserved", "persistence_end_ns"]


def _header():
    return open(os.path.join(ROOT, "include", "navgpu.h")).read()


def test_handover_record_layout_and_constants_match_header(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "sz.c"
    offs = ",".join(f"offsetof(navgpu_handover_record,{f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "navgpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %lld %lld %d\\n",'
                   'sizeof(navgpu_handover_record),' + offs + ',NAVGPU_HANDOVER_NONE,NAVGPU_HANDOVER_ADOPT,NAVGPU_HANDOVER_KEEP,'
                   'NAVGPU_HANDOVER_TOO_LONG,NAVGPU_PERSISTENCE_INITIAL,NAVGPU_PERSISTENCE_NEWPLAN,NAVGPU_MAX_POLYGON);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    H = _lib.HandoverRecord
    assert [n for n, _ in H._fields_] == FIELDS
    assert v[0] == C.sizeof(H) == 32
    assert v[1:8] == [getattr(H, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24]
    assert v[8:12] == [_lib.HANDOVER_NONE, _lib.HANDOVER_ADOPT, _lib.HANDOVER_KEEP, _lib.HANDOVER_TOO_LONG] == [0, 1, 2, 3]
    assert v[12:14] == [_lib.PERSISTENCE_INITIAL, _lib.PERSISTENCE_NEWPLAN] == [0, 1_000_000_000]  # ros::Time(0, 0), ros::Time(1, 0)
    assert v[14] == _lib.MAX_POLYGON >= 64


def test_plan_service_layouts_match_header(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "ps.c"
    rq = ["start", "goal", "frame", "tolerance", "default_tolerance"]
    rs = ["winner", "slot", "tried", "n_candidates", "n_poses", "rounds"]
    offs = ",".join([f"offsetof(navgpu_plan_service_request,{f})" for f in rq] + [f"offsetof(navgpu_plan_service_result,{f})" for f in rs])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "navgpu.h"\nint main(){size_t v[]={sizeof(navgpu_plan_service_request),'
                   'sizeof(navgpu_plan_service_result),NAVGPU_PLAN_SERVICE_MAX_CANDIDATES,' + offs + '};'
                   'for(unsigned i=0;i<sizeof v/sizeof*v;++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "ps"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Q, S = _lib.PlanServiceRequest, _lib.PlanServiceResult
    assert v[:3] == [C.sizeof(Q), C.sizeof(S), _lib.PLAN_SERVICE_MAX_CANDIDATES] == [88, 24, 1024]
    assert [n for n, _ in Q._fields_] == rq and [n for n, _ in S._fields_] == rs
    assert v[3:] == [getattr(Q, f).offset for f in rq] + [getattr(S, f).offset for f in rs]


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
    for name in ("set_polygon_cost", "clear_costmap_windows", "handover_global_plans", "reset_plan_persistence", "plan_persistence",
                 "set_plan_persistence"):
        assert callable(getattr(nav.Fleet, name))
    for name in ("plan_service", "plan_service_candidates", "set_costmap_from_fleet_instance"):
        assert callable(getattr(nav.NavFn, name))


def test_every_new_function_names_what_it_replaces():
    hdr = _header()
    cites = {"navgpu_costmap_set_polygon_cost": "costmap_2d.cpp:315-428", "navgpu_move_base_clear_costmap_windows": "move_base.cpp:277-330",
             "navgpu_move_base_handover_plans": "move_base.cpp:873-888", "navgpu_move_base_reset_persistence": "move_base.cpp:664",
             "navgpu_move_base_get_persistence": "persistence_end_", "navgpu_move_base_plan_service_candidates": "move_base.cpp:372-396",
             "navgpu_move_base_plan_service": "move_base.cpp:365-417", "navgpu_navfn_set_costmap_from_fleet_instance": "navfn_ros.cpp:265-268"}
    for name, cite in cites.items():
        at = hdr.index("int " + name + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "replaces:" in comment and cite in comment, name


def test_null_and_range_arguments_fail_without_a_device():
    """argument checks come before any device work"""
    import navigation_amd as nav
    L = nav.lib()
    off = (C.c_uint32 * 2)(0, 0)
    xy = (C.c_double * 2)(0, 0)
    st = (C.c_int64 * 1)(0)
    assert L.navgpu_costmap_set_polygon_cost(None, 0, 0, 1, None, off, 0, None) == -1
    assert L.navgpu_move_base_clear_costmap_windows(None, 0, 1, xy, 1.0, 1.0, None) == -1
    assert L.navgpu_move_base_handover_plans(None, 0, None, 0, 1, 0, None, xy, 0, 0, None) == -1
    assert L.navgpu_move_base_reset_persistence(None, 0, 1) == -1
    assert L.navgpu_move_base_get_persistence(None, 0, 1, st) == -1
    assert L.navgpu_move_base_set_persistence(None, 0, 1, st) == -1
