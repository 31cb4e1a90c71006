"""navgpu_amcl_node_integrate_odom (AmclNode::integrateOdom, amcl_node.cpp:1120-1172) and the node-state entry points against the
Python restatement of tests/amcl_node_ref.py.  The arithmetic is the host's, but a handle needs a device: marked gpu."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amcl_node_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if nav.lib().navgpu_device_count() <= 0:
        pytest.skip("no GPU")
    return nav


def track():
    """20 odometry messages: straight runs, a pure rotation, a step below 1e-6 m, strafing, and headings that wrap through +-pi"""
    p = [[1.0, 2.0, 3.0]]
    steps = [(0.05, 0.0, 0.02), (0.05, 0.01, 0.05), (0.0, 0.0, 0.3),        # 3rd: a pure rotation
             (3e-7, -2e-7, 0.01),                                           # delta_trans < 1e-6
             (0.04, 0.03, 0.08), (0.04, 0.03, 0.08),                        # the heading passes +pi here (3.0 + ... > pi)
             (-0.03, 0.05, -0.2), (-0.03, 0.05, -0.2), (-0.03, 0.05, -0.2), (-0.03, 0.05, -0.2),  # and back through -pi / +pi
             (0.0, 0.08, 0.0), (0.0, -0.08, 0.0),                           # strafe
             (0.1, 0.0, 3.0), (0.1, 0.0, 3.0),                              # turns close to pi per message
             (0.02, 0.02, -0.01), (0.0, 0.0, -0.6), (0.07, -0.01, 0.0), (0.07, -0.01, 0.4), (0.01, 0.0, 0.0)]
    for dx, dy, dth in steps:
        x, y, th = p[-1]
        p.append([x + dx, y + dy, th + dth])  # the yaw is left unwrapped on purpose: angle_diff normalises it
    p[6][2] -= 2 * math.pi                   # one message reports the wrapped heading
    assert len(p) == 20
    return p


def test_integrate_odom_matches_the_reference_lines(nav):
    a = nav.AmclLaser(2, 16, max_beams=8)
    r = ref.NodeRef(0.2, 0.5, 2, use_odom_integrator=True)
    poses = track()
    a.integrate_odom([poses[0], poses[0]])
    r.integrate_odom(poses[0])
    s = a.node_state()
    assert s.odom_integrator_ready.tolist() == [1, 1] and np.all(s.odom_integrator_absolute_motion == 0.0)
    seen_small = seen_rot = False
    for i in range(1, 20):
        a.integrate_odom([poses[i]], first=1)      # filter 1 alone; filter 0 must not move
        last = list(r.integrator_last_pose)
        r.integrate_odom(poses[i])
        s = a.node_state()
        got = s.odom_integrator_absolute_motion[1]
        d = math.hypot(poses[i][0] - last[0], poses[i][1] - last[1])
        seen_small |= d < 1e-6 and d > 0
        seen_rot |= d == 0.0
        # the rotation term: + - fabs and angle_diff's atan2 / sin / cos of the same arguments by the same libm
        assert abs(got[2] - r.absolute_motion[2]) <= 1e-12
        assert abs(got[0] - r.absolute_motion[0]) <= 1e-12 and abs(got[1] - r.absolute_motion[1]) <= 1e-12
        assert np.array_equal(s.odom_integrator_last_pose[1], np.array(poses[i]))   # a copy: equal
        assert np.array_equal(s.odom_integrator_last_pose[0], np.array(poses[0]))
        assert np.all(s.odom_integrator_absolute_motion[0] == 0.0)
    assert seen_small and seen_rot
    assert got[2] > 5.0 and got[0] > 0.2 and got[1] > 0.1   # the track did accumulate in all three
    a.close()


def test_below_1e6_takes_the_forward_branch_exactly(nav):
    """delta_trans < 1e-6: delta_bearing = 0, so the increments are fabs(delta_trans * 1) and fabs(delta_trans * 0): only
    + - * fabs sqrt are involved and the values are equal, not merely close"""
    a = nav.AmclLaser(1, 16, max_beams=8)
    a.integrate_odom([[0.0, 0.0, 0.0]])
    a.integrate_odom([[3e-7, 4e-7, 0.0]])
    m = a.node_state().odom_integrator_absolute_motion[0]
    assert m[0] == math.sqrt(3e-7 * 3e-7 + 4e-7 * 4e-7) and m[1] == 0.0 and m[2] == 0.0
    a.close()


def test_node_state_round_trip_reset_and_nomotion(nav):
    a = nav.AmclLaser(3, 16, max_beams=8)
    s = a.node_state()
    assert s.pf_init.tolist() == [0, 0, 0] and s.lasers_update.tolist() == [1, 1, 1] and s.force_update.tolist() == [0, 0, 0]
    assert s.latest_tf_valid.tolist() == [0, 0, 0] and s.global_localization_active.tolist() == [0, 0, 0]
    s.pf_init[:] = [1, 0, 7]            # any non-zero flag is stored as 1
    s.resample_count[:] = [5, 6, 7]
    s.pf_odom_pose[1] = [1.5, -2.5, 0.25]
    s.latest_tf[2] = [0.1, 0.2, 0.3]
    s.latest_tf_valid[2] = 1
    s.odom_integrator_last_pose[0] = [9.0, 8.0, 7.0]
    a.set_node_state(s)
    t = a.node_state()
    assert t.pf_init.tolist() == [1, 0, 1] and t.resample_count.tolist() == [5, 6, 7]
    assert t.pf_odom_pose[1].tolist() == [1.5, -2.5, 0.25] and t.latest_tf[2].tolist() == [0.1, 0.2, 0.3]
    assert t.odom_integrator_last_pose[0].tolist() == [9.0, 8.0, 7.0] and t.latest_tf_valid.tolist() == [0, 0, 1]
    a.request_nomotion_update(first=1, count=1)
    a.node_reset(global_localization=True, first=2, count=1)
    t = a.node_state()
    assert t.force_update.tolist() == [0, 1, 0]
    assert t.pf_init.tolist() == [1, 0, 0] and t.global_localization_active.tolist() == [0, 0, 1]
    assert t.resample_count.tolist() == [5, 6, 7]      # the reset touches nothing else
    a.node_reset(first=2, count=1)
    assert a.node_state().global_localization_active.tolist() == [0, 0, 0]
    a.close()
