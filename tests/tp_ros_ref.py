"""TrajectoryPlannerROS's host arithmetic restated in Python from base_local_planner/src/trajectory_planner_ros.cpp, line by line: the
stop / rotate candidates (:283-290, :312-337) and the branch logic, latch and flags of computeVelocityCommands (:372-526), setPlan
(:355-370) and isGoalReached (:590-597).  What the device answers - grids, findBestPath, scoreTrajectory - is not restated here: decide()
says which robots need which of them, and the tests get those answers from a twin fleet driven through the single entry points.
The window (transformGlobalPlan + prunePlan) is the caller's `window` function: the tests pass navgpu_local_plan_window, which has its
own tests.  Python floats are IEEE doubles, math.fmod / sqrt / hypot are the C library's: results are comparable with ==."""
import math

BRANCH_NONE, BRANCH_DWA, BRANCH_STOP, BRANCH_ROTATE, BRANCH_AT_GOAL, BRANCH_ROLLOUT = range(6)
NONE, ROLLOUT, REACHED, AT_GOAL = range(4)  # what a robot's cycle comes to


def sign(x):  # trajectory_planner_ros.h:192-194
    return -1.0 if x < 0.0 else 1.0


def normalize_angle(a):  # angles::normalize_angle, fmod form
    r = math.fmod(math.fmod(a, 2.0 * math.pi) + 2.0 * math.pi, 2.0 * math.pi)
    return r - 2.0 * math.pi if r > math.pi else r


def shortest_angular_distance(a, b):
    return normalize_angle(b - a)


def stopped(v, rot_stopped, trans_stopped):  # goal_functions.cpp:249-254
    return abs(v[2]) <= rot_stopped and abs(v[0]) <= trans_stopped and abs(v[1]) <= trans_stopped


def stop_candidate(cfg, odom_vel):
    """stopWithAccLimits (:283-290); cfg: dict or object with acc_lim_x, acc_lim_y, acc_lim_theta, sim_period."""
    g = cfg.get if isinstance(cfg, dict) else lambda k: getattr(cfg, k)
    vx = sign(odom_vel[0]) * max(0.0, (abs(odom_vel[0]) - g("acc_lim_x") * g("sim_period")))
    vy = sign(odom_vel[1]) * max(0.0, (abs(odom_vel[1]) - g("acc_lim_y") * g("sim_period")))
    vel_yaw = odom_vel[2]
    vth = sign(vel_yaw) * max(0.0, (abs(vel_yaw) - g("acc_lim_theta") * g("sim_period")))
    return (vx, vy, vth)


def rotate_candidate(cfg, yaw, vel_yaw, goal_th):
    """rotateToGoal (:312-337)"""
    g = cfg.get if isinstance(cfg, dict) else lambda k: getattr(cfg, k)
    max_vel_th, min_vel_th, min_in_place, acc, period = (g(k) for k in ("max_vel_th", "min_vel_th", "min_in_place_vel_th", "acc_lim_theta",
                                                                         "sim_period"))
    ang_diff = shortest_angular_distance(yaw, goal_th)
    v = min(max_vel_th, max(min_in_place, ang_diff)) if ang_diff > 0.0 else max(min_vel_th, min(-1.0 * min_in_place, ang_diff))
    max_acc_vel = abs(vel_yaw) + acc * period
    min_acc_vel = abs(vel_yaw) - acc * period
    v = sign(v) * min(max(abs(v), min_acc_vel), max_acc_vel)
    max_speed_to_stop = math.sqrt(2 * acc * abs(ang_diff))
    v = sign(v) * min(max_speed_to_stop, abs(v))
    v = min(max_vel_th, max(min_in_place, v)) if v > 0.0 else max(min_vel_th, min(-1.0 * min_in_place, v))
    return (0.0, 0.0, v)


class Robot:
    """The members of one TrajectoryPlannerROS that the cycle reads and writes."""

    def __init__(self):
        self.plan = []          # global_plan_: list of (x, y, yaw)
        self.T = None
        self.have_plan = False
        self.latch = self.rotating = self.reached = False

    def set_plan(self, plan, T=None):  # :355-370 (rotating_to_goal_ is not reset)
        self.plan = [tuple(float(v) for v in p) for p in plan]
        self.T = None if T is None else tuple(float(v) for v in T)
        self.have_plan = True
        self.latch = False
        self.reached = False


class Decision:
    def __init__(self):
        self.kind, self.branch, self.window, self.goal_th, self.candidate = NONE, BRANCH_NONE, [], 0.0, None


def decide(robots, params, cfg, poses, odom_vels, have_pose, window):
    """computeVelocityCommands up to the device's answers, for every robot.  params: xy_goal_tolerance, yaw_goal_tolerance,
    rot_stopped_velocity, trans_stopped_velocity, latch_xy_goal_tolerance, prune_plan (dict).  window(plan, pose, T, prune) ->
    (list of poses, n_erased).  Updates the robots' members; returns a Decision per robot."""
    out = []
    for r, pose, vel, have in zip(robots, poses, odom_vels, have_pose):
        d = Decision()
        out.append(d)
        if not have or not r.have_plan or not r.plan:  # :380-389
            continue
        win, n_erased = window(r.plan, pose, r.T, params["prune_plan"])
        if n_erased:  # prunePlan erases both plans in lockstep from their beginnings (:392-393)
            del r.plan[:n_erased]
        d.window = win
        if not win:  # :408-409
            continue
        goal_x, goal_y, d.goal_th = win[-1]  # transformed_plan.back() (:411-419)
        d.kind, d.branch = ROLLOUT, BRANCH_ROLLOUT
        if r.latch or math.hypot(goal_x - pose[0], goal_y - pose[1]) <= params["xy_goal_tolerance"]:  # :422
            if params["latch_xy_goal_tolerance"]:
                r.latch = True
            angle = shortest_angular_distance(pose[2], d.goal_th)
            if abs(angle) <= params["yaw_goal_tolerance"]:  # :432-439
                r.rotating = False
                r.latch = False
                r.reached = True
                d.kind, d.branch = AT_GOAL, BRANCH_AT_GOAL
            elif not r.rotating and not stopped(vel, params["rot_stopped_velocity"], params["trans_stopped_velocity"]):  # :452-456
                d.kind, d.branch, d.candidate = REACHED, BRANCH_STOP, stop_candidate(cfg, vel)
            else:  # :458-464
                r.rotating = True
                d.kind, d.branch, d.candidate = REACHED, BRANCH_ROTATE, rotate_candidate(cfg, pose[2], vel[2], d.goal_th)
    return out
