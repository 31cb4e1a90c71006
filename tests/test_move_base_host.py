"""tests/move_base_ref.py, the yardstick of the move_base GPU tests, pinned on the CPU against values worked out by hand from
move_base/src/move_base.cpp:372-396 and :784-836: planService's candidate goals - also the library's own host generator against the
yardstick's -, the persistence state table and findClosestPlanIndex's corner cases."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import move_base_ref as R  # noqa: E402

NOW, TIMEOUT = 50_000_000_000, 10_000_000_000
INITIAL, NEWPLAN = R.PERSISTENCE_INITIAL, R.PERSISTENCE_NEWPLAN


def test_special_states_are_the_reference_times():
    assert (INITIAL, NEWPLAN) == (0, 1_000_000_000)  # ros::Time(0, 0), ros::Time(1, 0)


def test_persistence_state_table():
    prefer = dict(controller_len=100, closest_i=20, new_len=80 + 321)  # prev_len 80: 80 + 320 < 401
    equal = dict(controller_len=100, closest_i=20, new_len=80 + 320)   # 80 + 320 < 400 is false
    rows = [  # state, lengths, (keep, state afterwards)
        (INITIAL, prefer, (False, NEWPLAN)),             # the first plan after a new goal is always taken
        (NEWPLAN, prefer, (True, NOW + TIMEOUT)),        # the timer starts with the first plan that is turned down
        (NOW + 5, prefer, (True, NOW + 5)),              # running: kept, the end stays
        (NOW, prefer, (False, NEWPLAN)),                 # now < end is false at the end itself
        (NOW - 1, prefer, (False, NEWPLAN)),             # expired
        (INITIAL, equal, (False, NEWPLAN)),
        (NEWPLAN, equal, (False, NEWPLAN)),
        (NOW + 5, equal, (False, NEWPLAN)),              # a plan that is not much longer ends a running preference
    ]
    for state, lens, want in rows:
        assert R.prefer_prev_plan(state, now=NOW, timeout=TIMEOUT, **lens) == want, (state, lens)
    assert R.prefer_prev_plan(NEWPLAN, 100, 20, 401, now=5, timeout=0) == (False, NEWPLAN)  # a timer of no length: 5 < 5 + 0 is false


def test_find_closest_plan_index():
    line = np.stack([np.arange(40) * 0.1, np.zeros(40)], 1)
    assert R.find_closest_plan_index(line, (1.21, 0.3)) == 12            # sampled indices only: 12, not 13
    assert R.find_closest_plan_index(line, (1.0, 0.3)) == 8              # 0.8 and 1.2 are equally far: the first
    assert R.find_closest_plan_index(line[:1], (7.0, 7.0)) == 0
    assert R.find_closest_plan_index(np.zeros((0, 2)), (7.0, 7.0)) == 0  # an empty plan
    far = line.copy()
    far[::4, 0] += 2e9
    assert R.find_closest_plan_index(far, (1.0, 0.0)) == 0               # nothing below min_dist = 1e9
    nan = line.copy()
    nan[8, 0] = np.nan
    assert R.find_closest_plan_index(nan, (0.8, 0.0)) in (4, 12) and R.find_closest_plan_index(nan, (0.79, 0.0)) == 4
    assert R.find_closest_plan_index(np.full((9, 2), np.nan), (0.0, 0.0)) == 0


def test_handover_record():
    line = np.stack([np.arange(500) * 0.01, np.zeros(500)], 1)
    got = R.handover(NEWPLAN, line, (1.0, 0.0), 900, NOW, TIMEOUT)
    assert got == dict(decision=R.KEEP, closest_index=100, prev_len=400, new_len=900, dropped=0, persistence_end_ns=NOW + TIMEOUT)
    got = R.handover(NEWPLAN, line, (1.0, 0.0), 720, NOW, TIMEOUT)
    assert got == dict(decision=R.ADOPT, closest_index=100, prev_len=400, new_len=720, dropped=0, persistence_end_ns=NEWPLAN)


def _ring(k):
    """candidates of ring k: the outer layer of a (k + 1) x (k + 1) quadrant, mirrored where an offset is not 0"""
    return 8 * k


def test_candidate_generator_counts_and_ends():
    f32 = np.float32
    g = (1.625, -0.375)
    inc = float(f32(float(f32(0.05)) * 3.0))  # (float)(resolution * 3.0)
    c = R.plan_service_candidates(g, 0.05, 0.5)  # three rings
    assert len(c) - 1 == 48 == _ring(1) + _ring(2) + _ring(3) and c[0] == g
    assert c[1] == (g[0] - inc, g[1]) and c[2] == (g[0] + inc, g[1])  # y_offset 0: one y_mult, x_offset = max_offset: both x_mult
    m3 = float(f32(f32(f32(inc) + f32(inc)) + f32(inc)))
    assert c[-1] == (g[0] + m3, g[1] + m3)
    # tolerance < increment: the increment becomes (float)tolerance.  (float)0.1 > 0.1, so `max_offset <= tolerance` fails at once and
    # the reference searches nothing; 0.125 is a float, and there is one ring at that offset
    assert R.plan_service_candidates(g, 0.05, 0.1) == [g]
    c = R.plan_service_candidates(g, 0.05, 0.125)
    assert len(c) - 1 == 8 and c[1] == (g[0] - 0.125, g[1]) and c[-1] == (g[0] + 0.125, g[1] + 0.125)
    # tolerance = 0 and tolerance < 0: max_offset <= tolerance never holds, the exact goal alone
    assert R.plan_service_candidates(g, 0.05, 0.0) == [g]
    assert R.plan_service_candidates(g, 0.05, -0.3) == [g]
    assert len(set(R.plan_service_candidates(g, 0.05, 0.5))) == 49  # no candidate twice


def test_library_candidates_are_the_yardsticks():
    import navigation_amd as nav
    from navigation_amd import _lib as N
    L = nav.lib()
    rs = np.random.RandomState(4)
    cases = [(0.05, 0.5), (0.05, 0.1), (0.05, 0.125), (0.05, 0.0), (0.05, -0.3), (0.05, 0.15), (0.025, 1.0), (0.1, 0.3), (0.05, float("nan"))]
    cases += [(float(rs.uniform(0.03, 0.2)), float(rs.uniform(0.0, 1.0))) for _ in range(30)]
    for res, tol in cases:
        g = rs.uniform(-20, 20, 2)
        want = np.asarray(R.plan_service_candidates(g, res, tol))
        n = L.navgpu_move_base_plan_service_candidates(g.ctypes.data, res, tol, 0, None)
        assert n == len(want), (res, tol, n, len(want))
        got = np.zeros((n, 2))
        assert L.navgpu_move_base_plan_service_candidates(g.ctypes.data, res, tol, n, got.ctypes.data) == n
        assert got.tobytes() == want.tobytes(), (res, tol)
    g = np.zeros(2)
    assert L.navgpu_move_base_plan_service_candidates(g.ctypes.data, 0.0, 0.5, 0, None) == -1
    assert L.navgpu_move_base_plan_service_candidates(None, 0.05, 0.5, 0, None) == -1
    assert L.navgpu_move_base_plan_service_candidates(g.ctypes.data, 0.001, 1.0, 0, None) == N.PLAN_SERVICE_MAX_CANDIDATES + 1  # the count stops there
    assert L.navgpu_move_base_plan_service(None, 0, 1, 1, 0, None, None, None, None, None, None) == -1


def test_service_loop():
    calls = []

    def make_plan(goal):
        calls.append(goal)
        return np.zeros((0, 3)) if len(calls) < 4 else np.array([[0.0, 0.0, 0.0], [goal[0], goal[1], goal[2]]])

    goal = (1.0, 2.0, 0.7)
    winner, tried, plan = R.plan_service(goal, 0.05, 0.5, make_plan)
    assert (winner, tried, len(calls)) == (3, 4, 4) and plan[-1].tolist() == list(goal) and len(plan) == 3
    assert calls[0] == goal and calls[3][2] == 0.7
    winner, tried, plan = R.plan_service(goal, 0.05, 0.5, lambda g: np.zeros((0, 3)))
    assert (winner, tried, len(plan)) == (-1, 49, 0)
    winner, tried, plan = R.plan_service(goal, 0.05, 0.5, lambda g: np.array([[g[0], g[1], g[2]]]))
    assert (winner, tried) == (0, 1) and len(plan) == 1  # the exact goal: nothing appended
