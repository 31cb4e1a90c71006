"""CPU-side checks of tests/obs_buffer_ref.py, the yardstick of tests/test_gpu_obs_buffer.py: the restatement of
costmap_2d::ObservationBuffer is pinned on cases worked by hand from the reference text (costmap_2d/src/observation_buffer.cpp:
purgeStaleObservations :211-236, bufferCloud :160-179, isCurrent :238-251; plugins/obstacle_layer.cpp:281-289).  No GPU."""
import math

import numpy as np

import obs_buffer_ref as R

F32 = np.float32
S = 1_000_000_000  # one second in ns


def _cloud(stamp, pts=((1.0, 0.0, 0.5),), **kw):
    return dict(instance=0, source=0, stamp_ns=stamp, points=np.array(pts, F32), **kw)


def test_keep_time_zero_keeps_one_entry():
    """:217-221: erase(++begin, end) - only the newest survives, whatever the stamps say"""
    b = R.RefList(dict(observation_keep_time_ns=0))
    b.buffer(_cloud(5 * S), 5 * S, R.host_trig)
    b.buffer(_cloud(1 * S, pts=((2.0, 0.0, 0.5),)), 6 * S, R.host_trig)  # an OLDER stamp arrives later: still the front
    assert [e["stamp"] for e in b.entries] == [1 * S]
    assert b.entries[0]["points"][0, 0] == 2.0


def test_keep_time_boundary_is_strict_and_takes_everything_behind():
    """:229: (last_updated - stamp) > keep_time.  keep 2 s, entries stamped 10, 9, 8 s (newest first)."""
    b = R.RefList(dict(observation_keep_time_ns=2 * S))
    for t in (8, 9, 10):
        b.buffer(_cloud(t * S), t * S, R.host_trig)
    assert [e["stamp"] for e in b.entries] == [10 * S, 9 * S, 8 * S]  # newest first; 10 - 8 = 2 is not > 2
    b.last_updated = 10 * S + 1  # one ns later the 8 s entry is 2 s + 1 ns old
    b.purge()
    assert [e["stamp"] for e in b.entries] == [10 * S, 9 * S]
    # an entry in the middle that is too old takes everything behind it with it, younger stamps included (:231)
    b = R.RefList(dict(observation_keep_time_ns=2 * S))
    b.buffer(_cloud(9 * S), 9 * S, R.host_trig)      # will sit behind the stale one
    b.buffer(_cloud(6 * S), 9 * S, R.host_trig)      # 9 - 6 = 3 > 2: erased at once, and the 9 s entry behind it too
    assert b.entries == []
    b.buffer(_cloud(9 * S), 9 * S, R.host_trig)
    b.buffer(_cloud(7 * S), 9 * S, R.host_trig)      # exactly at the boundary: stays, in front
    assert [e["stamp"] for e in b.entries] == [7 * S, 9 * S]


def test_is_current_is_inclusive():
    """:243: (now - last_updated) <= expected_update_rate; 0 means always"""
    b = R.RefList(dict(expected_update_rate_ns=S // 2))
    b.buffer(_cloud(0), 10 * S, R.host_trig)
    assert b.is_current(10 * S + S // 2) and not b.is_current(10 * S + S // 2 + 1)
    assert R.RefList(dict(expected_update_rate_ns=0)).is_current(10 ** 18)


def test_height_bounds_inclusive_at_both_ends_and_nan_drops():
    """:169-170: z <= max && z >= min"""
    pts = [(0, 0, 0.25), (1, 0, 0.2499), (2, 0, 1.5), (3, 0, 1.5001), (4, 0, float("nan")), (5, 0, 1.0)]
    b = R.RefList(dict(min_obstacle_height=0.25, max_obstacle_height=1.5))
    b.buffer(_cloud(0, pts=pts), 0, R.host_trig)
    assert b.entries[0]["points"][:, 0].tolist() == [0.0, 2.0, 5.0]  # cloud order
    assert b.entries[0]["n_unfiltered"] == 6
    # the comparison is in double on the float z: 0.1f > 0.1, so a minimum of 0.1 keeps it and a maximum of 0.1 does not
    assert len(R.height_filter(np.array([[0, 0, 0.1]], F32), 0.1, 2.0)) == 1
    assert len(R.height_filter(np.array([[0, 0, 0.1]], F32), 0.0, 0.1)) == 0


def test_cloud_transform_order_and_narrowing():
    """fp32, left to right: ((m00 x + m01 y) + m02 z) + m03 - a case where the order shows"""
    m = [1, 1, 1, 0, 1, 0, 0, 0, 1, 0, 0.5, 0]
    p = np.array([[2.0 ** 24, 1.0, -(2.0 ** 24)]], F32)
    out = R.transform_cloud(m, p)
    assert out[0, 0] == 0.0  # (2^24 + 1) rounds to 2^24 in fp32; right to left it would be 1
    assert out[0, 1] == 1.5 and out[0, 2] == -(2.0 ** 24)
    out = R.transform_cloud([0.1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.array([[9.0, 0, 0]], F32))
    assert out[0, 0] == F32(0.1) * F32(9.0) and out[0, 0] != F32(0.1 * 9.0)  # the matrix is narrowed BEFORE the product


def test_scan_inf_rule_and_range_tests():
    """obstacle_layer.cpp:281-289 and projectLaser's range test: r >= range_min && r < range_max"""
    inf, nan = float("inf"), float("nan")
    rmin, rmax = 0.5, 4.0
    just_under = np.nextafter(F32(rmax), F32(0))
    ranges = np.array([1.0, inf, -inf, nan, 0.4999, 0.5, rmax, just_under, 2.0], F32)
    pts, idx = R.project_scan(ranges, -0.3, 0.1, rmin, rmax, 0, R.host_trig)
    assert idx.tolist() == [0, 5, 7, 8]  # +inf without the flag drops, range_min is inclusive, range_max exclusive
    pts1, idx1 = R.project_scan(ranges, -0.3, 0.1, rmin, rmax, 1, R.host_trig)
    assert idx1.tolist() == [0, 1, 5, 7, 8]  # +inf becomes range_max - 0.0001f, which passes; -inf and NaN never do
    r_inf = F32(rmax) - F32(0.0001)
    a1 = float(F32(-0.3)) + 1.0 * float(F32(0.1))  # the angles are the float fields promoted to double
    assert pts1[1, 0] == F32(float(r_inf) * math.cos(a1)) and pts1[1, 1] == F32(float(r_inf) * math.sin(a1)) and pts1[1, 2] == 0.0
    a8 = float(F32(-0.3)) + 8.0 * float(F32(0.1))
    assert pts[3, 0] == F32(2.0 * math.cos(a8)) and pts[3, 1] == F32(2.0 * math.sin(a8))
    # where 0.0001 is below half an ulp of range_max the substitute IS range_max and fails the test, as in the reference
    _, idx2 = R.project_scan(np.array([inf], F32), 0.0, 0.1, 0.5, 4096.0, 1, R.host_trig)
    assert idx2.tolist() == []


def test_fleet_order_eviction_and_set_global_frame():
    src = [dict(observation_keep_time_ns=10 * S, flags=1), dict(observation_keep_time_ns=10 * S, flags=2, raytrace_range=7.0)]
    fb = R.RefObsBuf(2, src, slots=2)
    fb.buffer([dict(instance=1, source=1, stamp_ns=1 * S, points=[(1, 0, 1)], origin=(1, 2, 3)),
               dict(instance=1, source=0, stamp_ns=2 * S, points=[(2, 0, 1)]),
               dict(instance=1, source=1, stamp_ns=3 * S, points=[(3, 0, 1)]),
               dict(instance=1, source=1, stamp_ns=4 * S, points=[(4, 0, 1)])], 4 * S)
    obs = fb.observations(1)
    # sources in configuration order, each newest first; the third cloud of source 1 pushed its oldest out
    assert [(o["flags"], o["points"][0, 0]) for o in obs] == [(1, 2.0), (2, 4.0), (2, 3.0)]
    assert fb.evicted == [0, 1] and fb.observations(0) == [] and obs[1]["raytrace_range"] == 7.0
    # setGlobalFrame: a quarter turn about z and a shift; origins in fp64, points in fp32, nothing filtered again
    fb.set_global_frame([0, -1, 0, 1, 0, 0, 0, 0, 1, 10, 20, 30])
    obs = fb.observations(1)
    assert obs[1]["points"].tolist() == [[10.0, 24.0, 31.0]] and obs[1]["origin"] == (10.0, 20.0, 30.0)
    fb2 = R.RefObsBuf(1, [dict(max_obstacle_height=2.0)], slots=1)
    fb2.buffer([dict(instance=0, stamp_ns=0, points=[(0, 0, 1)])], 0)
    fb2.set_global_frame([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 5])
    assert fb2.observations(0)[0]["points"][0, 2] == 6.0  # above max_obstacle_height now, and kept
