"""CPU-side checks of the legacy planner's fleet entry points (navgpu_tp_update_plans, navgpu_tp_score_trajectories, navgpu_tp_ros_*):
declared, exported and bound; the new struct and enum value as the C compiler sees include/navgpu.h against the Python mirrors; argument
errors that need no device; and the pure host function navgpu_tp_ros_candidate against the Python restatement of stopWithAccLimits /
rotateToGoal in tests/tp_ros_ref.py, as doubles.  No GPU."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tp_ros_ref as R  # noqa: E402

NAMES = {"navgpu_tp_update_plans": 6, "navgpu_tp_score_trajectories": 7, "navgpu_tp_ros_configure": 2, "navgpu_tp_ros_set_plans": 6,
         "navgpu_tp_ros_compute_velocity_commands": 5, "navgpu_tp_ros_is_goal_reached": 4, "navgpu_tp_ros_check_trajectories": 9,
         "navgpu_tp_ros_get_plan": 4, "navgpu_tp_ros_transformed_plan": 4, "navgpu_tp_ros_candidate": 6}
METHODS = ("tp_update_plans", "tp_score_trajectories", "configure_tp_ros", "tp_ros_set_plans", "tp_ros_compute_velocity_commands",
           "tp_ros_is_goal_reached", "tp_ros_check_trajectories", "tp_ros_global_plan", "tp_ros_transformed_plan")


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
    # the single calls keep their signatures
    assert len(bound["navgpu_tp_update_plan"]) == 5 and len(bound["navgpu_tp_score_trajectory"]) == 6


def test_struct_size_branch_and_kernel_count_match_header(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "tpros.c"  # as C: the header is a C header
    src.write_text('#include <stdio.h>\n#include "navgpu.h"\nint main(){printf("%zu %d %d %d\\n", sizeof(navgpu_tp_ros_params), '
                   'NAVGPU_BRANCH_ROLLOUT, NAVGPU_BRANCH_AT_GOAL, NAVGPU_K_COUNT);return 0;}\n')
    exe = tmp_path / "tpros"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, rollout, at_goal, k_count = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(_lib.TpRosParams)
    assert rollout == 5 == _lib.BRANCH_ROLLOUT == R.BRANCH_ROLLOUT and at_goal == 4 == _lib.BRANCH_AT_GOAL
    assert k_count == 10 == len(_lib.KERNELS)  # k_tp_probe is timed under NAVGPU_K_SCORE: no new kernel id
    p = _lib.TpRosParams()
    assert (p.xy_goal_tolerance, p.yaw_goal_tolerance, p.rot_stopped_velocity, p.trans_stopped_velocity, p.latch_xy_goal_tolerance,
            p.prune_plan) == (0.10, 0.05, 1e-2, 1e-2, 0, 1)


def test_argument_errors_need_no_gpu(nav):
    """argument checks come before anything touches a device"""
    L = nav.lib()
    u32 = lambda *v: np.asarray(v, np.uint32)  # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    inst, off, dec_inst, dec_off = u32(0, 1), u32(0, 1, 2), u32(1, 0), u32(0, 2, 1)
    probes, costs = np.zeros((2, 9)), np.zeros(2)
    assert L.navgpu_tp_update_plans(None, 0, 1, None, p(u32(0, 0)), 0) == -1
    assert L.navgpu_tp_score_trajectories(None, 1, None, None, None, None, None) == -1
    assert L.navgpu_tp_score_trajectories(None, 2, p(inst), p(off), p(probes), p(costs), None) == -1
    assert L.navgpu_tp_score_trajectories(None, 2, p(dec_inst), p(off), p(probes), p(costs), None) == -1
    assert L.navgpu_tp_score_trajectories(None, 2, p(inst), p(dec_off), p(probes), p(costs), None) == -1
    assert L.navgpu_tp_ros_configure(None, None) == -1
    assert L.navgpu_tp_ros_set_plans(None, 0, 1, None, p(u32(0, 0)), None) == -1
    assert L.navgpu_tp_ros_compute_velocity_commands(None, 0, 1, None, None) == -1
    assert L.navgpu_tp_ros_is_goal_reached(None, 0, 1, None) == -1
    assert L.navgpu_tp_ros_check_trajectories(None, 2, p(dec_inst), None, p(dec_off), None, 0, None, None) == -1
    assert L.navgpu_tp_ros_get_plan(None, 0, None, 0) == -1 and L.navgpu_tp_ros_transformed_plan(None, 0, None, 0) == -1
    assert L.navgpu_tp_ros_candidate(None, 0, None, None, 0.0, None) == -1


def _candidate(L, cfg, rotate, pose, vel, goal_th):
    out = np.zeros(3)
    a, b = np.asarray(pose, np.float64), np.asarray(vel, np.float64)
    assert L.navgpu_tp_ros_candidate(C.byref(cfg), rotate, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), float(goal_th),
                                     out.ctypes.data_as(C.c_void_p)) == 0
    return tuple(float(v) for v in out)


CONFIGS = (dict(), dict(acc_lim_theta=0.4, min_in_place_vel_th=0.7, max_vel_th=0.9, min_vel_th=-0.8, sim_period=0.1),
           dict(acc_lim_x=0.3, acc_lim_y=9.0, acc_lim_theta=20.0, min_in_place_vel_th=0.0))


@pytest.mark.parametrize("kw", CONFIGS)
def test_candidates_equal_the_restatement(nav, kw):
    from navigation_amd import _lib
    L = nav.lib()
    cfg = _lib.TpConfig(**kw)
    assert L.navgpu_shortest_angular_distance(0.3, 2.9) == R.shortest_angular_distance(0.3, 2.9)
    n = overridden = 0
    for yaw, vel_yaw, ang_diff in itertools.product((0.0, 0.3, -2.9), (0.0, 0.05, -0.05, 1.0, -1.0), (0.0, 1e-3, -1e-3, 0.3, -0.3, 3.0, -3.0)):
        goal_th = yaw + ang_diff
        got = _candidate(L, cfg, 1, (1.0, 2.0, yaw), (0.2, -0.1, vel_yaw), goal_th)
        want = R.rotate_candidate(cfg, yaw, vel_yaw, goal_th)
        assert got == want, (kw, yaw, vel_yaw, ang_diff, got, want)
        assert got[0] == 0.0 and got[1] == 0.0 and cfg.min_vel_th <= got[2] <= cfg.max_vel_th
        # min_in_place_vel_th against the acceleration limit: what the robot can reach in one period is less, the floor wins
        if cfg.min_in_place_vel_th > abs(vel_yaw) + cfg.acc_lim_theta * cfg.sim_period:
            assert abs(got[2]) == cfg.min_in_place_vel_th
            overridden += 1
        n += 1
    assert n == 105 and (overridden > 0 or cfg.min_in_place_vel_th == 0.0)
    for vx, vy, vel_yaw in itertools.product((0.0, 0.3, -0.3, 0.05), (0.0, -0.2, 0.01), (0.0, 0.05, -0.05, 1.0, -1.0)):
        got = _candidate(L, cfg, 0, (1.0, 2.0, 0.3), (vx, vy, vel_yaw), 0.0)
        want = R.stop_candidate(cfg, (vx, vy, vel_yaw))
        assert got == want, (kw, vx, vy, vel_yaw, got, want)
        assert all(abs(g) <= abs(v) for g, v in zip(got, (vx, vy, vel_yaw)))


def test_min_in_place_overrides_the_acceleration_limit_and_zero_difference(nav):
    """the two cases the grid must hold, by hand (BaseLocalPlanner.cfg defaults: acc_lim_theta 3.2, sim_period 0.05, floor 0.4)"""
    from navigation_amd import _lib
    L = nav.lib()
    cfg = _lib.TpConfig()
    # stopped, 0.3 rad to go: one period allows 0.16 rad/s, the floor commands 0.4
    assert _candidate(L, cfg, 1, (0, 0, 0.0), (0, 0, 0.0), 0.3) == (0.0, 0.0, 0.4) == R.rotate_candidate(cfg, 0.0, 0.0, 0.3)
    # ang_diff == 0 takes the negative branch (:319-321): -min_in_place_vel_th
    assert _candidate(L, cfg, 1, (0, 0, 0.7), (0, 0, 0.0), 0.7) == (0.0, 0.0, -0.4) == R.rotate_candidate(cfg, 0.7, 0.0, 0.7)
