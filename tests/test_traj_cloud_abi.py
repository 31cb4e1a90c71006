"""CPU-side checks of the trajectory-cloud part of the C-ABI: the ctypes mirror of navgpu_sample_terms agrees with include/navgpu.h
field by field (sizeof and offsetof as the C compiler sees them), so does the numpy record Fleet.sample_terms returns, the constant
agrees, and the three entry points are declared, exported and bound, and check their arguments before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("navgpu_planner_set_trajectory_cloud", "navgpu_planner_trajectory_cloud", "navgpu_planner_sample_terms")


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    return nav


def test_struct_layout_matches_header(tmp_path):
    from navigation_amd import _lib
    from navigation_amd.fleet import Fleet
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "navgpu.h"', 'int main(){',
             'printf("size %zu\\n", sizeof(navgpu_sample_terms));']
    for field, _ in _lib.SampleTerms._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(navgpu_sample_terms, {field}));')
    lines.append('printf("max_robots %d\\n", NAVGPU_TRAJ_CLOUD_MAX_ROBOTS);')
    lines.append('return 0;}')
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    dt = Fleet.SAMPLE_TERMS_DTYPE
    assert int(out["size"]) == C.sizeof(_lib.SampleTerms) == dt.itemsize == 80
    for field, _ in _lib.SampleTerms._fields_:
        assert int(out[field]) == getattr(_lib.SampleTerms, field).offset == dt.fields[field][1], field
    assert tuple(dt.names) == tuple(f for f, _ in _lib.SampleTerms._fields_)
    assert dt.fields["critic"][0].shape == (5,) and dt.fields["critic"][0].base == np.float64
    assert int(out["max_robots"]) == _lib.TRAJ_CLOUD_MAX_ROBOTS == 16


def test_entry_points_are_declared_exported_and_bound(nav):
    from navigation_amd import _lib
    L = nav.lib()
    header = open(os.path.join(ROOT, "include", "navgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    cites = {"navgpu_planner_set_trajectory_cloud": "dwa_planner.cpp:160-163", "navgpu_planner_trajectory_cloud": "dwa_planner.cpp:318-348",
             "navgpu_planner_sample_terms": "simple_scored_sampling_planner.cpp:50-79"}
    for name in ENTRY_POINTS:
        m = re.search(r"\bint " + name + r"\(", header)
        assert m, name
        assert hasattr(L, name) and name in bound, name
        # every entry point cites the reference lines it replaces, in the comment (and struct) that leads up to it
        before = header[:m.start()]
        lead = before[before.rindex(";\n", 0, before.rindex("/*", 0, before.rindex("*/"))) if name != "navgpu_planner_sample_terms" else before.rindex("int navgpu_planner_trajectory_cloud("):]
        assert cites[name] in lead, name
    for method in ("set_trajectory_cloud", "trajectory_cloud", "sample_terms"):
        assert callable(getattr(nav.Fleet, method))


def test_argument_errors_need_no_gpu(nav):
    L = nav.lib()
    assert L.navgpu_planner_set_trajectory_cloud(None, 0, 1, 1) == -1
    assert L.navgpu_planner_trajectory_cloud(None, 0, 1, None, 0) == -1
    assert L.navgpu_planner_sample_terms(None, 0, None, 0) == -1


def test_plugin_header_offers_the_cloud():
    hdr = open(os.path.join(ROOT, "navigation_amd", "plugin", "navgpu_dwa_planner_ros.h")).read()
    src = open(os.path.join(ROOT, "navigation_amd", "plugin", "navgpu_dwa_planner_ros.cpp")).read()
    assert "navgpu_planner_trajectory_cloud" in hdr and "std::vector<float> trajectoryCloud()" in hdr
    assert '"publish_traj_pc"' in src and "navgpu_planner_set_trajectory_cloud" in src
    assert "advertise" not in src  # the adapter publishes nothing
