"""The yardstick of the move_base tests: an independent restatement, in Python, of the lines of move_base/src/move_base.cpp that
navgpu_move_base_* replaces (move_base needs ROS and cannot be compiled for the tests; the footing of oracle/local_planner_oracle.py).

  find_closest_plan_index   MoveBase::findClosestPlanIndex (:784-799), distances by numpy.hypot - the host's libm, which is what the
                            reference calls; math.hypot is CPython's own algorithm
  prefer_prev_plan          MoveBase::preferPrevPlan (:808-836) on integer nanoseconds
  plan_service_candidates   planService's goal search (:372-396) in numpy.float32 loop variables, as written
  plan_service              the loop round them (:365-417) over a make_plan callback
"""
import numpy as np

PERSISTENCE_INITIAL = 0              # ros::Time(0, 0)
PERSISTENCE_NEWPLAN = 1_000_000_000  # ros::Time(1, 0)
ADOPT, KEEP = 1, 2


def sampled_distances(plan_xy, pos_xy):
    """distance(current_position, plan[i]) for i = 0, 4, 8, ..."""
    p = np.asarray(plan_xy, np.float64).reshape(-1, 2)[::4]
    return np.hypot(np.float64(pos_xy[0]) - p[:, 0], np.float64(pos_xy[1]) - p[:, 1])


def find_closest_plan_index(plan_xy, pos_xy):
    closest_i, min_dist = 0, 1000000000.0
    with np.errstate(invalid="ignore", over="ignore"):
        d = sampled_distances(plan_xy, pos_xy)
    for j in range(len(d)):
        if d[j] < min_dist:
            min_dist = d[j]
            closest_i = 4 * j
    return closest_i


def prefer_prev_plan(state, controller_len, closest_i, new_len, now, timeout):
    """-> (prefer the previous plan, the new persistence_end_)"""
    prev_plan_len = controller_len - closest_i
    prefer_prev = prev_plan_len + 320 < new_len
    if prefer_prev and state != PERSISTENCE_INITIAL:
        if state == PERSISTENCE_NEWPLAN:
            state = now + timeout
        if now < state:
            return True, state
    return False, PERSISTENCE_NEWPLAN


def handover(state, controller_xy, pos_xy, new_len, now, timeout):
    """one robot whose new plan was made -> dict of navgpu_handover_record's fields (dropped 0)"""
    controller_xy = np.asarray(controller_xy, np.float64).reshape(-1, 2)
    ci = find_closest_plan_index(controller_xy, pos_xy)
    keep, state = prefer_prev_plan(state, len(controller_xy), ci, new_len, now, timeout)
    return dict(decision=KEEP if keep else ADOPT, closest_index=ci, prev_len=len(controller_xy) - ci, new_len=new_len, dropped=0,
                persistence_end_ns=state)


def plan_service_candidates(goal_xy, resolution, tolerance):
    """the goals planService tries, in its order; candidate 0 is the exact goal.  Every float variable of the reference is a
    numpy.float32 here, every mixed expression is promoted to float64 as C++ promotes it."""
    f32, f64 = np.float32, np.float64
    gx, gy = f64(goal_xy[0]), f64(goal_xy[1])
    out = [(float(gx), float(gy))]
    resolution = f32(resolution)                 # float resolution = ...->getResolution();
    search_increment = f32(f64(resolution) * 3.0)  # float search_increment = resolution*3.0;
    tol = f64(tolerance)
    if tol > 0.0 and tol < f64(search_increment):
        search_increment = f32(tol)
    if not search_increment > 0:  # (the reference's loops would not end)
        return out
    eps = f64(1e-9)
    max_offset = search_increment
    while f64(max_offset) <= tol:
        y_offset = f32(0)
        while y_offset <= max_offset:
            x_offset = f32(0)
            while x_offset <= max_offset:
                if not (f64(x_offset) < f64(max_offset) - eps and f64(y_offset) < f64(max_offset) - eps):
                    y_mult = f32(-1.0)
                    while f64(y_mult) <= 1.0 + eps:
                        if not (f64(y_offset) < eps and f64(y_mult) < -1.0 + eps):
                            x_mult = f32(-1.0)
                            while f64(x_mult) <= 1.0 + eps:
                                if not (f64(x_offset) < eps and f64(x_mult) < -1.0 + eps):
                                    out.append((float(gx + f64(f32(x_offset * x_mult))), float(gy + f64(f32(y_offset * y_mult)))))
                                x_mult = f32(f64(x_mult) + 2.0)
                        y_mult = f32(f64(y_mult) + 2.0)
                x_offset = f32(x_offset + search_increment)
            y_offset = f32(y_offset + search_increment)
        max_offset = f32(max_offset + search_increment)
    return out


def plan_service(goal_xyyaw, resolution, tolerance, make_plan):
    """make_plan(goal_xyyaw) -> (n, 3) poses, empty when it fails.  -> (winner or -1, makePlan calls made, the plan)"""
    cands = plan_service_candidates(goal_xyyaw[:2], resolution, tolerance)
    for i, (x, y) in enumerate(cands):
        plan = np.asarray(make_plan((x, y, float(goal_xyyaw[2]))), np.float64).reshape(-1, 3)
        if len(plan):
            if i:  # global_plan.push_back(req.goal)
                plan = np.concatenate([plan, np.asarray(goal_xyyaw, np.float64).reshape(1, 3)])
            return i, i + 1, plan
    return -1, len(cands), np.zeros((0, 3))
