"""ctypes declarations for include/navgpu.h (one-to-one)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

LAYER_STATIC, LAYER_OBSTACLE, LAYER_VOXEL, LAYER_INFLATION = 1, 2, 4, 8
GRID_MASTER, GRID_STATIC, GRID_OBSTACLE, GRID_VOXEL, GRID_PATH, GRID_GOAL, GRID_GOAL_FRONT = range(7)
OBS_MARKING, OBS_CLEARING = 1, 2
VOXEL_UNKNOWN, VOXEL_MARKED = 1, 2  # voxel_grid::VoxelStatus
K_OBSTACLE, K_MERGE, K_INFLATE, K_BFS, K_SCORE, K_SELECT, K_FOOTPRINT, K_VOXEL_EXPORT, K_OBS_INGEST, K_CHECK_TRAJ = range(10)
KERNELS = ("k_obstacle", "k_merge", "k_inflate", "k_bfs", "k_score", "k_select", "k_footprint_cost", "k_voxel_export", "k_obs_ingest", "k_check_traj")
CLOUD_XYZ, CLOUD_SCAN = 0, 1  # NAVGPU_CLOUD_*
OBSBUF_MAX_SOURCES, OBSBUF_MAX_CLOUD_POINTS = 8, 65536


class NavgpuError(RuntimeError):
    pass


class FleetDesc(C.Structure):
    _fields_ = [("n_instances", C.c_uint32), ("size_x", C.c_uint32), ("size_y", C.c_uint32),
                ("resolution", C.c_double), ("layers", C.c_int32), ("track_unknown", C.c_int32),
                ("device", C.c_int32), ("max_points", C.c_uint32), ("max_observations", C.c_uint32),
                ("max_plan", C.c_uint32), ("max_footprint", C.c_uint32), ("max_sim_steps", C.c_uint32),
                ("keep_sample_costs", C.c_int32), ("rolling_window", C.c_int32)]


class Observation(C.Structure):
    _fields_ = [("instance", C.c_uint32), ("first_point", C.c_uint32), ("n_points", C.c_uint32),
                ("flags", C.c_uint32), ("origin_x", C.c_double), ("origin_y", C.c_double),
                ("origin_z", C.c_double), ("obstacle_range", C.c_double), ("raytrace_range", C.c_double)]


class ObsSourceParams(C.Structure):
    """Mirror of navgpu_obs_source_params (include/navgpu.h): one entry of observation_sources.  Defaults: obstacle_layer.cpp:96-140."""
    _fields_ = [("observation_keep_time_ns", C.c_int64), ("expected_update_rate_ns", C.c_int64), ("min_obstacle_height", C.c_double),
                ("max_obstacle_height", C.c_double), ("obstacle_range", C.c_double), ("raytrace_range", C.c_double), ("flags", C.c_uint32),
                ("inf_is_valid", C.c_int32)]
    DEFAULTS = dict(observation_keep_time_ns=0, expected_update_rate_ns=0, min_obstacle_height=0.0, max_obstacle_height=2.0,
                    obstacle_range=2.5, raytrace_range=3.0, flags=OBS_MARKING | OBS_CLEARING, inf_is_valid=0)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


class Cloud(C.Structure):
    """Mirror of navgpu_cloud (include/navgpu.h): one cloud or scan of a navgpu_obsbuf_buffer call."""
    _fields_ = [("instance", C.c_uint32), ("source", C.c_uint32), ("kind", C.c_uint32), ("first", C.c_uint32), ("n", C.c_uint32),
                ("reserved", C.c_uint32), ("stamp_ns", C.c_int64), ("origin", C.c_double * 3), ("transform", C.c_double * 12),
                ("angle_min", C.c_float), ("angle_increment", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float)]


class ObsBufRobotStatus(C.Structure):
    """Mirror of navgpu_obsbuf_robot_status (include/navgpu.h)."""
    _fields_ = [("kept", C.c_uint32), ("points", C.c_uint32), ("evicted", C.c_uint64), ("current", C.c_int32), ("reserved", C.c_int32)]


class ObstacleParams(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("footprint_clearing_enabled", C.c_int32),
                ("combination_method", C.c_int32), ("z_voxels", C.c_int32), ("max_obstacle_height", C.c_double),
                ("origin_z", C.c_double), ("z_resolution", C.c_double), ("unknown_threshold", C.c_int32),
                ("mark_threshold", C.c_int32)]


class InflationParams(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("priority_queue_order", C.c_int32), ("inflation_radius", C.c_double),
                ("cost_scaling_factor", C.c_double), ("inscribed_radius", C.c_double)]


class DwaConfig(C.Structure):
    """navgpu_dwa_config; defaults are the reference's (DWAPlanner.cfg:15-36, local_planner_limits)."""
    _fields_ = [(n, C.c_double) for n in (
        "max_trans_vel", "min_trans_vel", "max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y",
        "max_rot_vel", "min_rot_vel", "acc_lim_x", "acc_lim_y", "acc_lim_theta",
        "sim_time", "sim_granularity", "angular_sim_granularity", "sim_period",
        "path_distance_bias", "goal_distance_bias", "occdist_scale",
        "forward_point_distance", "cheat_factor", "oscillation_reset_dist", "oscillation_reset_angle")] + [
        (n, C.c_int32) for n in (
            "vx_samples", "vy_samples", "vth_samples", "use_dwa", "discretize_by_time", "sum_scores",
            "allow_unknown", "rollout_trig")]

    DEFAULTS = dict(max_trans_vel=0.55, min_trans_vel=0.1, max_vel_x=0.55, min_vel_x=0.0, max_vel_y=0.1,
                    min_vel_y=-0.1, max_rot_vel=1.0, min_rot_vel=0.4, acc_lim_x=2.5, acc_lim_y=2.5,
                    acc_lim_theta=3.2, sim_time=1.7, sim_granularity=0.025, angular_sim_granularity=0.1,
                    sim_period=0.05, path_distance_bias=32.0, goal_distance_bias=24.0, occdist_scale=0.01,
                    forward_point_distance=0.325, cheat_factor=1.0, oscillation_reset_dist=0.05,
                    oscillation_reset_angle=0.2, vx_samples=3, vy_samples=10, vth_samples=20, use_dwa=1,
                    discretize_by_time=0, sum_scores=0, allow_unknown=1, rollout_trig=0)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RobotState(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("vel", C.c_float * 3), ("plan_first", C.c_uint32),
                ("plan_count", C.c_uint32)]


class PlanResult(C.Structure):
    _fields_ = [("best_index", C.c_int32), ("n_samples", C.c_int32), ("n_scored", C.c_int32),
                ("n_valid", C.c_int32), ("n_points", C.c_int32), ("oscillation_flags", C.c_uint32),
                ("xv", C.c_float), ("yv", C.c_float), ("thetav", C.c_float), ("reserved", C.c_float),
                ("cost", C.c_double), ("drive", C.c_double * 3)]


TRAJ_CLOUD_MAX_ROBOTS = 16


class SampleTerms(C.Structure):
    """navgpu_sample_terms: one sample slot of an enabled robot's last cycle (navgpu_planner_sample_terms)."""
    _fields_ = [("critic", C.c_double * 5), ("cost_full", C.c_double), ("cost_ref", C.c_double), ("first_fail", C.c_int32),
                ("status", C.c_int32), ("n_points", C.c_int32), ("member", C.c_int32), ("point_offset", C.c_uint32),
                ("reserved", C.c_uint32)]


class LocalLimits(C.Structure):
    _fields_ = [("xy_goal_tolerance", C.c_double), ("yaw_goal_tolerance", C.c_double), ("rot_stopped_vel", C.c_double),
                ("trans_stopped_vel", C.c_double), ("max_rot_vel", C.c_double), ("min_rot_vel", C.c_double),
                ("acc_lim_x", C.c_double), ("acc_lim_y", C.c_double), ("acc_lim_theta", C.c_double),
                ("sim_period", C.c_double), ("prune_plan", C.c_int32), ("latch_xy_goal_tolerance", C.c_int32)]


class RobotLimits(C.Structure):
    """navgpu_robot_limits: base_local_planner::LocalPlannerLimits of one robot (navgpu_planner_set_limits)."""
    _fields_ = [(n, C.c_double) for n in (
        "max_trans_vel", "min_trans_vel", "max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y",
        "max_rot_vel", "min_rot_vel", "acc_lim_x", "acc_lim_y", "acc_lim_theta",
        "xy_goal_tolerance", "yaw_goal_tolerance", "trans_stopped_vel", "rot_stopped_vel")] + [
        ("prune_plan", C.c_int32), ("reserved", C.c_int32)]
    FIELDS = tuple(n for n, _ in _fields_[:-1])  # what a caller's record names; `reserved` is the library's

    def as_dict(self):
        return {n: getattr(self, n) for n in self.FIELDS}


class RobotInput(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("odom_vel", C.c_double * 3), ("have_pose", C.c_int32), ("reserved", C.c_int32)]


class CmdResult(C.Structure):
    _fields_ = [("cmd_vel", C.c_double * 3), ("ok", C.c_int32), ("branch", C.c_int32), ("local_plan_points", C.c_int32),
                ("trajectory_points", C.c_int32)]


BRANCH_NONE, BRANCH_DWA, BRANCH_STOP, BRANCH_ROTATE, BRANCH_AT_GOAL, BRANCH_ROLLOUT = range(6)


class LocalWindow(C.Structure):
    """Mirror of navgpu_local_window (include/navgpu.h): what getLocalPlan did for one robot in the last cycle."""
    _fields_ = [("first_index", C.c_int32), ("n_window", C.c_int32), ("n_erased", C.c_int32), ("n_local", C.c_int32),
                ("remaining", C.c_int32), ("status", C.c_int32)]


LOCAL_WINDOW_OK, LOCAL_WINDOW_NONE, LOCAL_WINDOW_CAPACITY = range(3)  # navgpu_local_window_status
PLAN_FAMILY_GLOBAL_PLANNER, PLAN_FAMILY_NAVFN_ROS = range(2)  # navgpu_plan_family


class HandoverRecord(C.Structure):
    """Mirror of navgpu_handover_record (include/navgpu.h): what MoveBase::preferPrevPlan decided for one robot."""
    _fields_ = [("decision", C.c_int32), ("closest_index", C.c_int32), ("prev_len", C.c_int32), ("new_len", C.c_int32),
                ("dropped", C.c_int32), ("reserved", C.c_int32), ("persistence_end_ns", C.c_int64)]


class PlanServiceRequest(C.Structure):
    """Mirror of navgpu_plan_service_request (include/navgpu.h): one nav_msgs::GetPlan request of MoveBase::planService."""
    _fields_ = [("start", C.c_double * 3), ("goal", C.c_double * 3), ("frame", C.c_double * 3), ("tolerance", C.c_double),
                ("default_tolerance", C.c_double)]


class PlanServiceResult(C.Structure):
    """Mirror of navgpu_plan_service_result (include/navgpu.h)."""
    _fields_ = [("winner", C.c_int32), ("slot", C.c_int32), ("tried", C.c_int32), ("n_candidates", C.c_int32), ("n_poses", C.c_int32),
                ("rounds", C.c_int32)]


PLAN_SERVICE_MAX_CANDIDATES = 1024  # NAVGPU_PLAN_SERVICE_MAX_CANDIDATES
HANDOVER_NONE, HANDOVER_ADOPT, HANDOVER_KEEP, HANDOVER_TOO_LONG = range(4)  # navgpu_handover_decision
PERSISTENCE_INITIAL, PERSISTENCE_NEWPLAN = 0, 1000000000  # MoveBase::persistence_end_'s special values, ns
MAX_POLYGON = 256  # NAVGPU_MAX_POLYGON


class TpConfig(C.Structure):
    """navgpu_tp_config; defaults are BaseLocalPlanner.cfg's (base_local_planner/cfg/BaseLocalPlanner.cfg)."""
    _fields_ = [(n, C.c_double) for n in (
        "acc_lim_x", "acc_lim_y", "acc_lim_theta", "sim_time", "sim_granularity", "angular_sim_granularity",
        "pdist_scale", "gdist_scale", "occdist_scale", "heading_lookahead", "oscillation_reset_dist",
        "escape_reset_dist", "escape_reset_theta", "max_vel_x", "min_vel_x", "max_vel_th", "min_vel_th",
        "min_in_place_vel_th", "backup_vel", "sim_period", "heading_scoring_timestep")] + [("y_vels", C.c_double * 8)] + [
        (n, C.c_int32) for n in ("n_y_vels", "vx_samples", "vtheta_samples", "holonomic_robot", "dwa", "allow_unknown",
                                 "heading_scoring", "simple_attractor")]

    DEFAULTS = dict(acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2, sim_time=1.7, sim_granularity=0.025,
                    angular_sim_granularity=0.025, pdist_scale=0.6, gdist_scale=0.8, occdist_scale=0.01,
                    heading_lookahead=0.325, oscillation_reset_dist=0.05, escape_reset_dist=0.10,
                    escape_reset_theta=1.5707963267948966, max_vel_x=0.55, min_vel_x=0.0, max_vel_th=1.0, min_vel_th=-1.0,
                    min_in_place_vel_th=0.4, backup_vel=-0.1, sim_period=0.05, heading_scoring_timestep=0.1,
                    y_vels=(-0.3, -0.1, 0.1, 0.3),
                    vx_samples=20, vtheta_samples=20, holonomic_robot=1, dwa=0, allow_unknown=1, heading_scoring=0,
                    simple_attractor=0)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        yv = list(d.pop("y_vels"))
        d.pop("n_y_vels", None)
        for k, v in d.items():
            setattr(self, k, v)
        self.n_y_vels = len(yv)
        for i, v in enumerate(yv):
            self.y_vels[i] = float(v)

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("y_vels", "n_y_vels")}
        d["y_vels"] = tuple(self.y_vels[i] for i in range(self.n_y_vels))
        return d


class TpRosParams(C.Structure):
    """navgpu_tp_ros_params; defaults are TrajectoryPlannerROS's own (trajectory_planner_ros.cpp:97-98, 116-126)."""
    _fields_ = [("xy_goal_tolerance", C.c_double), ("yaw_goal_tolerance", C.c_double), ("rot_stopped_velocity", C.c_double),
                ("trans_stopped_velocity", C.c_double), ("latch_xy_goal_tolerance", C.c_int32), ("prune_plan", C.c_int32)]

    def __init__(self, xy_goal_tolerance=0.10, yaw_goal_tolerance=0.05, rot_stopped_velocity=1e-2, trans_stopped_velocity=1e-2,
                 latch_xy_goal_tolerance=0, prune_plan=1):
        super().__init__(xy_goal_tolerance, yaw_goal_tolerance, rot_stopped_velocity, trans_stopped_velocity, int(latch_xy_goal_tolerance),
                         int(prune_plan))


class TpState(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("prev_x", C.c_double), ("prev_y", C.c_double),
                ("escape_x", C.c_double), ("escape_y", C.c_double), ("escape_theta", C.c_double)]


class TpResult(C.Structure):
    _fields_ = [("xv", C.c_double), ("yv", C.c_double), ("thetav", C.c_double), ("cost", C.c_double), ("drive", C.c_double * 3),
                ("n_points", C.c_int32), ("n_samples", C.c_int32), ("best_sample", C.c_int32), ("reserved", C.c_int32)]


class TpSample(C.Structure):
    _fields_ = [("vx", C.c_double), ("vy", C.c_double), ("vtheta", C.c_double), ("cost", C.c_double), ("n_points", C.c_int32),
                ("reserved", C.c_int32)]


ROTATE_RUNNING, ROTATE_DONE, ROTATE_BLOCKED = range(3)
ROTATE_RECOVERY_MAX_SWEEP = 4096


class RotateRecoveryParams(C.Structure):
    """navgpu_rotate_recovery_params; defaults are the reference's (rotate_recovery.cpp:60-66)."""
    _fields_ = [(n, C.c_double) for n in ("sim_granularity", "acc_lim_th", "max_rotational_vel", "min_in_place_rotational_vel",
                                          "yaw_goal_tolerance")] + [("allow_unknown", C.c_int32), ("reserved", C.c_int32)]
    DEFAULTS = dict(sim_granularity=0.017, acc_lim_th=3.2, max_rotational_vel=1.0, min_in_place_rotational_vel=0.4,
                    yaw_goal_tolerance=0.10, allow_unknown=0, reserved=0)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


class RotateRecoveryState(C.Structure):
    _fields_ = [("start_offset", C.c_double), ("got_180", C.c_int32), ("started", C.c_int32), ("swept", C.c_int32),
                ("reserved", C.c_int32)]


class NavfnResult(C.Structure):
    """Mirror of navgpu_navfn_result (include/navgpu.h)."""
    _fields_ = [("found", C.c_int32), ("path_length", C.c_int32), ("cycles", C.c_int32), ("start_potential", C.c_float)]


class GlobalPlannerParams(C.Structure):
    """Mirror of navgpu_global_planner_params (include/navgpu.h); defaults = GlobalPlanner.cfg / planner_core.cpp:105-152."""
    _fields_ = [("use_dijkstra", C.c_int32), ("use_quadratic", C.c_int32), ("use_grid_path", C.c_int32), ("old_navfn_behavior", C.c_int32),
                ("allow_unknown", C.c_int32), ("lethal_cost", C.c_int32), ("neutral_cost", C.c_int32), ("cost_factor", C.c_float),
                ("outline_map", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        d = dict(use_dijkstra=1, use_quadratic=1, use_grid_path=0, old_navfn_behavior=0, allow_unknown=1, lethal_cost=253, neutral_cost=50,
                 cost_factor=3.0, outline_map=1, reserved=0)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


ORIENT_NONE, ORIENT_FORWARD, ORIENT_INTERPOLATE, ORIENT_FORWARD_THEN_INTERPOLATE = range(4)  # NAVGPU_ORIENT_*
MAKE_PLAN_OK, MAKE_PLAN_START_OFF_MAP, MAKE_PLAN_GOAL_OFF_MAP, MAKE_PLAN_NO_PLAN, MAKE_PLAN_BORDER = range(5)  # NAVGPU_MAKE_PLAN_*


class GlobalPose(C.Structure):
    """Mirror of navgpu_global_pose (include/navgpu.h)."""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double)]


class MakePlanOptions(C.Structure):
    """Mirror of navgpu_make_plan_options (include/navgpu.h)."""
    _fields_ = [("orientation_mode", C.c_int32), ("wavefront", C.c_int32)]


class MakePlanResult(C.Structure):
    """Mirror of navgpu_make_plan_result (include/navgpu.h)."""
    _fields_ = [("status", C.c_int32), ("n_poses", C.c_int32), ("found", C.c_int32), ("cycles", C.c_int32), ("start_cell", C.c_int32 * 2),
                ("goal_cell", C.c_int32 * 2), ("start_potential", C.c_float), ("reserved", C.c_int32)]


class NavfnRosParams(C.Structure):
    """Mirror of navgpu_navfn_ros_params (include/navgpu.h); defaults = NavfnROS.cfg's weights."""
    _fields_ = [("tolerance_weight_dist_from_goal", C.c_double), ("tolerance_weight_path_length", C.c_double), ("wavefront", C.c_int32),
                ("reserved", C.c_int32)]


class NavfnRosResult(C.Structure):
    """Mirror of navgpu_navfn_ros_result (include/navgpu.h)."""
    _fields_ = [("status", C.c_int32), ("n_poses", C.c_int32), ("found", C.c_int32), ("cycles", C.c_int32), ("start_cell", C.c_int32 * 2),
                ("goal_cell", C.c_int32 * 2), ("best_cell", C.c_int32 * 2), ("candidates", C.c_int32), ("start_potential", C.c_float),
                ("best_x", C.c_double), ("best_y", C.c_double), ("best_cost", C.c_double)]


class NavfnRosCloudPoint(C.Structure):
    """Mirror of navgpu_navfn_ros_cloud_point (include/navgpu.h)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("pot_value", C.c_float)]


NAVFN_ROS_MAX_WINDOW = 4096  # NAVGPU_NAVFN_ROS_MAX_WINDOW


AMCL_MODEL_BEAM, AMCL_MODEL_LIKELIHOOD_FIELD, AMCL_MODEL_LIKELIHOOD_FIELD_PROB, AMCL_MODEL_LIKELIHOOD_FIELD_GOMPERTZ = range(4)


class AmclLaserParams(C.Structure):
    """Mirror of navgpu_amcl_laser_params (include/navgpu.h).  Defaults: amcl_node.cpp's parameter defaults (likelihood field,
    max_beams 30, laser_z_* 0.95 / 0.1 / 0.05 / 0.05, laser_sigma_hit 0.2, laser_lambda_short 0.1, beam skip 0.5 / 0.3 / 0.9,
    alpha_slow / alpha_fast 0.001 / 0.1) and SetMapFactors' constructor values 1.0 / 1.0 / 0.0."""
    _fields_ = [("model_type", C.c_int32), ("max_beams", C.c_int32)] + [(n, C.c_double) for n in (
        "z_hit", "z_short", "z_max", "z_rand", "sigma_hit", "lambda_short", "chi_outlier")] + [
        ("do_beamskip", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_double) for n in (
            "beam_skip_distance", "beam_skip_threshold", "beam_skip_error_threshold", "gompertz_a", "gompertz_b", "gompertz_c",
            "input_shift", "input_scale", "output_shift", "off_map_factor", "non_free_space_factor", "non_free_space_radius",
            "alpha_slow", "alpha_fast")]

    DEFAULTS = dict(model_type=AMCL_MODEL_LIKELIHOOD_FIELD, max_beams=30, z_hit=0.95, z_short=0.1, z_max=0.05, z_rand=0.05, sigma_hit=0.2,
                    lambda_short=0.1, chi_outlier=0.0, do_beamskip=0, reserved=0, beam_skip_distance=0.5, beam_skip_threshold=0.3,
                    beam_skip_error_threshold=0.9, gompertz_a=1.0, gompertz_b=1.0, gompertz_c=1.0, input_shift=0.0, input_scale=1.0,
                    output_shift=0.0, off_map_factor=1.0, non_free_space_factor=1.0, non_free_space_radius=0.0, alpha_slow=0.001,
                    alpha_fast=0.1)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


AMCL_RESAMPLE_MULTINOMIAL, AMCL_RESAMPLE_SYSTEMATIC = range(2)
AMCL_DRAW_SUPPLIED, AMCL_DRAW_DEVICE = range(2)


class AmclResampleParams(C.Structure):
    """Mirror of navgpu_amcl_resample_params (include/navgpu.h).  Defaults: pf_alloc's pop_err 0.01, pop_z 3, dist_threshold 0.5
    (pf.c:72-74), amcl_node's min_particles 100 and its default multinomial resample_model."""
    _fields_ = [("resample_model", C.c_int32), ("min_samples", C.c_int32), ("pop_err", C.c_double), ("pop_z", C.c_double),
                ("dist_threshold", C.c_double)]
    DEFAULTS = dict(resample_model=AMCL_RESAMPLE_MULTINOMIAL, min_samples=100, pop_err=0.01, pop_z=3.0, dist_threshold=0.5)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


AMCL_ODOM_DIFF, AMCL_ODOM_OMNI, AMCL_ODOM_DIFF_CORRECTED, AMCL_ODOM_OMNI_CORRECTED, AMCL_ODOM_GAUSSIAN = range(5)
AMCL_DRAW_DRAND48 = 2


class AmclUniformParams(C.Structure):
    """Mirror of navgpu_amcl_uniform_params (include/navgpu.h): uniform_pose_starting_weight_threshold,
    uniform_pose_deweight_multiplier and the per-filter candidate cap (0: 100 x max_samples)."""
    _fields_ = [("starting_weight_threshold", C.c_double), ("deweight_multiplier", C.c_double), ("max_candidates", C.c_uint64)]


class AmclOdomParams(C.Structure):
    """Mirror of navgpu_amcl_odom_params (include/navgpu.h): odom_model_t and AMCLOdom's alpha1..alpha5.  Defaults: amcl_node's
    odom_model_type "diff" and odom_alpha1..5 0.2 (amcl_node.cpp)."""
    _fields_ = [("model_type", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_double) for n in (
        "alpha1", "alpha2", "alpha3", "alpha4", "alpha5")]
    DEFAULTS = dict(model_type=AMCL_ODOM_DIFF, reserved=0, alpha1=0.2, alpha2=0.2, alpha3=0.2, alpha4=0.2, alpha5=0.2)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


class AmclNodeParams(C.Structure):
    """Mirror of navgpu_amcl_node_params (include/navgpu.h).  Defaults: amcl_node's update_min_d 0.2, update_min_a pi / 6,
    resample_interval 2, laser_min_range / laser_max_range -1 (unset) and no odom integrator topic."""
    _fields_ = [("d_thresh", C.c_double), ("a_thresh", C.c_double), ("laser_min_range", C.c_double), ("laser_max_range", C.c_double),
                ("resample_interval", C.c_int32), ("use_odom_integrator", C.c_int32)]
    DEFAULTS = dict(d_thresh=0.2, a_thresh=0.5235987755982988, laser_min_range=-1.0, laser_max_range=-1.0, resample_interval=2,
                    use_odom_integrator=0)

    def __init__(self, **kw):
        super().__init__()
        d = dict(self.DEFAULTS)
        d.update(kw)
        for k, v in d.items():
            setattr(self, k, v)


AMCL_SCAN_PRESENT = 1  # NAVGPU_AMCL_SCAN_PRESENT


class AmclScan(C.Structure):
    """Mirror of navgpu_amcl_scan (include/navgpu.h)."""
    _fields_ = [("flags", C.c_uint32), ("range_count", C.c_uint32), ("range_offset", C.c_uint32), ("range_min", C.c_float),
                ("range_max", C.c_float), ("reserved", C.c_uint32), ("yaw_min", C.c_double), ("yaw_inc", C.c_double),
                ("odom_pose", C.c_double * 3)]


class AmclNodeResult(C.Structure):
    """Mirror of navgpu_amcl_node_result (include/navgpu.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "status", "moved", "updated", "resampled", "cloud_due", "published", "republish", "global_localization_converged",
        "sample_count", "converged", "cluster_count", "max_weight_hyp")] + [
        ("max_weight", C.c_double), ("pose", C.c_double * 3)] + [(n, C.c_double) for n in (
            "cov_xx", "cov_xy", "cov_yx", "cov_yy", "cov_aa")] + [("map_to_odom", C.c_double * 3)]


class AmclNodeState(C.Structure):
    """Mirror of navgpu_amcl_node_state (include/navgpu.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "pf_init", "lasers_update", "force_update", "resample_count", "odom_integrator_ready", "global_localization_active",
        "latest_tf_valid", "reserved")] + [(n, C.c_double * 3) for n in (
            "pf_odom_pose", "odom_integrator_absolute_motion", "odom_integrator_last_pose", "latest_tf")]


class Costmap3DDesc(C.Structure):
    """Mirror of navgpu_costmap3d_desc (include/navgpu.h)."""
    _fields_ = [("n_instances", C.c_uint32), ("size_x", C.c_uint32), ("size_y", C.c_uint32), ("size_z", C.c_uint32), ("resolution", C.c_double),
                ("max_triangles", C.c_uint32), ("max_boxes", C.c_uint32), ("max_poses", C.c_uint32), ("device", C.c_int32)]


class C3dBox(C.Structure):
    """Mirror of navgpu_c3d_box (include/navgpu.h)."""
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("cz", C.c_double), ("size", C.c_double), ("cls", C.c_int32), ("reserved", C.c_int32)]


class C3dRun(C.Structure):
    """Mirror of navgpu_c3d_run (include/navgpu.h)."""
    _fields_ = [("instance", C.c_uint32), ("first_pose", C.c_uint32), ("n_poses", C.c_uint32)]


class C3dRunResult(C.Structure):
    """Mirror of navgpu_c3d_run_result (include/navgpu.h)."""
    _fields_ = [("cost", C.c_double), ("n_lethal", C.c_int32), ("first_lethal", C.c_int32), ("n_done", C.c_int32), ("reserved", C.c_int32)]


C3D_MAX_TRIANGLES = 384
C3D_LETHAL, C3D_NONLETHAL = 0, 1
C3D_REPLACE, C3D_MARK, C3D_CLEAR = 0, 1, 2
C3D_COST, C3D_COLLISION_ONLY, C3D_DISTANCE = 0, 1, 2
C3D_REGION_ALL, C3D_REGION_LEFT, C3D_REGION_RIGHT, C3D_REGION_RECTANGULAR_PRISM = 0, 1, 2, 3


class C3dLayer(C.Structure):
    """Mirror of navgpu_c3d_layer (include/navgpu_costmap3d_layers.h)."""
    _fields_ = [("kind", C.c_int32), ("enabled", C.c_int32), ("combination_method", C.c_int32), ("cloud_has_intensity", C.c_int32),
                ("free_intensity", C.c_float), ("lethal_intensity", C.c_float), ("lethal_cost_threshold", C.c_int32),
                ("unknown_to_lethal", C.c_int32), ("height", C.c_double), ("radius", C.c_double), ("max_cloud_points", C.c_uint32),
                ("reserved", C.c_uint32)]


class C3dCloud(C.Structure):
    """Mirror of navgpu_c3d_cloud (include/navgpu_costmap3d_layers.h)."""
    _fields_ = [("instance", C.c_uint32), ("layer", C.c_uint32), ("first_point", C.c_uint32), ("n_points", C.c_uint32), ("transform", C.c_double * 12)]


C3D_MAX_LAYERS = 8
C3D_LAYER_POINT_CLOUD, C3D_LAYER_STATIC_2D, C3D_LAYER_CYLINDER_CLEARING = 0, 1, 2
C3D_COMBINE_OVERWRITE, C3D_COMBINE_MAXIMUM, C3D_COMBINE_IF_UNKNOWN, C3D_COMBINE_NOTHING = 0, 1, 2, 99
C3D_ROLL_CENTRE, C3D_ROLL_ORIGIN = 0, 1  # include/navgpu_costmap3d_rolling.h


class C3dLeaf(C.Structure):
    """Mirror of navgpu_c3d_leaf (include/navgpu_costmap3d_publish.h)."""
    _fields_ = [("key", C.c_int32 * 3), ("level", C.c_uint16), ("cls", C.c_uint16)]


class C3dUpdateMsg(C.Structure):
    """Mirror of navgpu_c3d_update_msg (include/navgpu_costmap3d_publish.h)."""
    _fields_ = [("instance", C.c_uint32), ("update_seq", C.c_uint32), ("bounds_seq", C.c_uint32), ("universe", C.c_int32), ("plain_map", C.c_int32),
                ("first_value", C.c_uint32), ("n_values", C.c_uint32), ("first_bound", C.c_uint32), ("n_bounds", C.c_uint32),
                ("n_forgotten", C.c_uint32), ("forgotten", (C.c_int32 * 6) * 2)]


C3D_FREE = 2  # include/navgpu_costmap3d_publish.h
C3D_EXPORT_FULL, C3D_EXPORT_DELTA = 0, 1
C3D_CELLS_BINARY, C3D_CELLS_AS_GIVEN = 0, 1
C3D_APPLIED, C3D_IGNORED, C3D_RESYNC = 0, 1, 2


def lib_path():
    return os.path.join(_HERE, "libnavgpu.so")


def build():
    """hipcc --offload-arch=gfx950 build of libnavgpu.so (cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc")], check=True)


# every symbol include/navgpu.h declares: (name, restype, argtypes)
vp, u32, i32, dbl = C.c_void_p, C.c_uint32, C.c_int32, C.c_double
SYMBOLS = [
    ("navgpu_version", C.c_char_p, []),
    ("navgpu_strerror", C.c_char_p, [C.c_int]),
    ("navgpu_last_error", C.c_char_p, []),
    ("navgpu_device_count", C.c_int, []),
    ("navgpu_fleet_create", C.c_int, [C.POINTER(FleetDesc), C.POINTER(vp)]),
    ("navgpu_fleet_destroy", C.c_int, [vp]),
    ("navgpu_sync", C.c_int, [vp]),
    ("navgpu_fleet_set_alloc_limit", C.c_int, [vp, C.c_uint64]),
    ("navgpu_stream", vp, [vp]),
    ("navgpu_fleet_set_origin", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_fleet_get_origin", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_grid_upload", C.c_int, [vp, C.c_int, u32, u32, vp]),
    ("navgpu_grid_download", C.c_int, [vp, C.c_int, u32, u32, vp]),
    ("navgpu_grid_device", C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]),
    ("navgpu_grid_reset", C.c_int, [vp, C.c_int, u32, u32]),
    ("navgpu_grid_reset_window", C.c_int, [vp, C.c_int, u32, u32, u32, u32, u32, u32]),
    ("navgpu_layer_reset_bounding_box", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_static_set_map", C.c_int, [vp, u32, u32, vp, i32, i32, i32, i32, i32]),
    ("navgpu_static_set_rolling_map", C.c_int, [vp, vp, u32, u32, C.c_double, C.c_double, C.c_double, i32, i32, i32, i32, i32]),
    ("navgpu_static_set_transform", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_obstacle_configure", C.c_int, [vp, C.POINTER(ObstacleParams)]),
    ("navgpu_inflation_configure", C.c_int, [vp, C.POINTER(InflationParams)]),
    ("navgpu_set_footprint", C.c_int, [vp, u32, u32, vp, u32]),
    ("navgpu_costmap_stage", C.c_int, [vp, u32, u32, vp, vp, u32, vp, u32]),
    ("navgpu_costmap_update", C.c_int, [vp, u32, u32]),
    ("navgpu_costmap_bounds", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_costmap_stage_list", C.c_int, [vp, u32, vp, vp, vp, u32, vp, u32]),
    ("navgpu_costmap_update_list", C.c_int, [vp, u32, vp]),
    ("navgpu_costmap_bounds_list", C.c_int, [vp, u32, vp, vp]),
    ("navgpu_inflate", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_obstacle_update_bounds", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_obstacle_update_costs", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_planner_configure", C.c_int, [vp, C.POINTER(DwaConfig)]),
    ("navgpu_planner_set_limits", C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
    ("navgpu_planner_get_limits", C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
    ("navgpu_planner_set_plan", C.c_int, [vp, u32, u32]),
    ("navgpu_planner_stage", C.c_int, [vp, u32, u32, vp, vp, u32]),
    ("navgpu_planner_stage_poses", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_planner_cycle", C.c_int, [vp, u32, u32]),
    ("navgpu_planner_set_bounded_map_grids", C.c_int, [vp, C.c_int32]),
    ("navgpu_planner_set_seed_lists", C.c_int, [vp, C.c_int32]),
    ("navgpu_planner_set_split_prep", C.c_int, [vp, C.c_int32]),
    ("navgpu_planner_set_seed_list_capacity", C.c_int, [vp, u32]),
    ("navgpu_planner_seed_list_counts", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_planner_set_map_grid_options", C.c_int, [vp, C.c_int32, C.c_int32, C.c_double]),
    ("navgpu_planner_wavefront_levels", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_planner_wavefront_boxes", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_planner_results", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_planner_set_cycles_in_flight", C.c_int, [vp, C.c_int32]),
    ("navgpu_planner_results_previous", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_planner_trajectory", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_planner_samples", C.c_int, [vp, u32, vp, vp, vp, u32]),
    ("navgpu_planner_check_trajectory", C.c_int, [vp, u32, vp, C.POINTER(i32)]),
    ("navgpu_planner_check_trajectories", C.c_int, [vp, u32, vp, vp, vp, vp, vp]),
    ("navgpu_planner_stage_list", C.c_int, [vp, u32, vp, vp, vp, u32]),
    ("navgpu_planner_stage_poses_list", C.c_int, [vp, u32, vp, vp, vp]),
    ("navgpu_planner_cycle_list", C.c_int, [vp, u32, vp]),
    ("navgpu_planner_results_list", C.c_int, [vp, u32, vp, vp]),
    ("navgpu_planner_cost_cloud", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_planner_set_trajectory_cloud", C.c_int, [vp, u32, u32, i32]),
    ("navgpu_planner_trajectory_cloud", C.c_int, [vp, u32, i32, vp, u32]),
    ("navgpu_planner_sample_terms", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_planner_get_oscillation", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_planner_set_oscillation", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_local_plan_window", C.c_int, [vp, u32, vp, vp, dbl, i32, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
    ("navgpu_shortest_angular_distance", dbl, [dbl, dbl]),
    ("navgpu_local_planner_configure", C.c_int, [vp, C.POINTER(LocalLimits)]),
    ("navgpu_local_planner_set_plan", C.c_int, [vp, u32, vp, u32, vp]),
    ("navgpu_local_planner_compute_velocity_commands", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_local_planner_is_goal_reached", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_local_planner_get_plan", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_local_planner_reserve_plans", C.c_int, [vp, u32]),
    ("navgpu_local_planner_set_plans", C.c_int, [vp, u32, u32, vp, vp, vp]),
    ("navgpu_local_planner_adopt_plans", C.c_int, [vp, u32, vp, u32, u32, i32, vp, vp]),
    ("navgpu_local_planner_local_plan", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_local_planner_windows", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_costmap_set_polygon_cost", C.c_int, [vp, C.c_int, u32, u32, vp, vp, C.c_uint8, vp]),
    ("navgpu_move_base_clear_costmap_windows", C.c_int, [vp, u32, u32, vp, C.c_double, C.c_double, vp]),
    ("navgpu_move_base_handover_plans", C.c_int, [vp, u32, vp, u32, u32, i32, vp, vp, C.c_int64, C.c_int64, vp]),
    ("navgpu_move_base_reset_persistence", C.c_int, [vp, u32, u32]),
    ("navgpu_move_base_get_persistence", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_move_base_set_persistence", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_move_base_plan_service_candidates", C.c_int, [vp, C.c_double, C.c_double, u32, vp]),
    ("navgpu_move_base_plan_service", C.c_int, [vp, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp]),
    ("navgpu_navfn_set_costmap_from_fleet_instance", C.c_int, [vp, u32, u32, vp, u32, i32, i32]),
    ("navgpu_tp_configure", C.c_int, [vp, C.POINTER(TpConfig)]),
    ("navgpu_tp_update_plan", C.c_int, [vp, u32, vp, u32, i32]),
    ("navgpu_tp_find_best_path", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_tp_trajectory", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_tp_samples", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_tp_score_trajectory", C.c_int, [vp, u32, vp, vp, vp, C.POINTER(dbl)]),
    ("navgpu_tp_get_state", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_tp_set_state", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_tp_update_plans", C.c_int, [vp, u32, u32, vp, vp, i32]),
    ("navgpu_tp_score_trajectories", C.c_int, [vp, u32, vp, vp, vp, vp, vp]),
    ("navgpu_tp_update_plans_list", C.c_int, [vp, u32, vp, vp, vp, i32]),
    ("navgpu_tp_find_best_path_list", C.c_int, [vp, u32, vp, vp, vp]),
    ("navgpu_tp_ros_configure", C.c_int, [vp, C.POINTER(TpRosParams)]),
    ("navgpu_tp_ros_set_plans", C.c_int, [vp, u32, u32, vp, vp, vp]),
    ("navgpu_tp_ros_compute_velocity_commands", C.c_int, [vp, u32, u32, vp, vp]),
    ("navgpu_tp_ros_is_goal_reached", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_tp_ros_check_trajectories", C.c_int, [vp, u32, vp, vp, vp, vp, i32, vp, vp]),
    ("navgpu_tp_ros_get_plan", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_tp_ros_transformed_plan", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_tp_ros_candidate", C.c_int, [C.POINTER(TpConfig), i32, vp, vp, dbl, vp]),
    ("navgpu_footprint_cost", C.c_int, [vp, u32, u32, vp, vp, i32, vp, vp]),
    ("navgpu_rotate_recovery_configure", C.c_int, [vp, C.POINTER(RotateRecoveryParams)]),
    ("navgpu_rotate_recovery_step", C.c_int, [vp, u32, u32, vp, vp, vp, vp]),
    ("navgpu_carrot_plan", C.c_int, [vp, u32, u32, vp, vp, i32, vp, vp]),
    ("navgpu_voxel_points", C.c_int, [vp, u32, u32, C.c_int, C.c_int, u32, vp, vp]),
    ("navgpu_voxel_clearing_endpoints", C.c_int, [vp, u32, u32, u32, vp, vp, vp]),
    ("navgpu_obsbuf_configure", C.c_int, [vp, vp, u32, u32, u32]),
    ("navgpu_obsbuf_buffer", C.c_int, [vp, vp, u32, vp, u32, vp, u32, C.c_int64]),
    ("navgpu_obsbuf_stage", C.c_int, [vp, u32, u32, vp, C.c_int64, vp]),
    ("navgpu_obsbuf_stage_list", C.c_int, [vp, u32, vp, vp, C.c_int64, vp]),
    ("navgpu_obsbuf_observations", C.c_int, [vp, u32, C.c_int64, vp, u32, vp, u32, C.POINTER(u32)]),
    ("navgpu_obsbuf_set_global_frame", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_obsbuf_reset_last_updated", C.c_int, [vp, u32, u32, C.c_int64]),
    ("navgpu_obsbuf_status", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_navfn_create", C.c_int, [u32, u32, u32, i32, C.POINTER(vp)]),
    ("navgpu_navfn_destroy", C.c_int, [vp]),
    ("navgpu_navfn_set_costmap", C.c_int, [vp, u32, u32, vp, i32, i32, i32]),
    ("navgpu_navfn_set_costmap_from_fleet", C.c_int, [vp, u32, u32, vp, u32, i32]),
    ("navgpu_navfn_plan", C.c_int, [vp, u32, u32, vp, vp, i32, i32, vp]),
    ("navgpu_navfn_plan_wavefront", C.c_int, [vp, u32, u32, vp, vp, i32, vp]),
    ("navgpu_global_planner_plan", C.c_int, [vp, u32, u32, C.POINTER(GlobalPlannerParams), vp, vp, vp, vp]),
    ("navgpu_global_planner_plan_wavefront", C.c_int, [vp, u32, u32, C.POINTER(GlobalPlannerParams), vp, vp, vp, vp]),
    ("navgpu_global_planner_make_plan", C.c_int, [vp, u32, u32, C.POINTER(GlobalPlannerParams), C.POINTER(MakePlanOptions), vp, vp, vp, vp]),
    ("navgpu_global_planner_plans", C.c_int, [vp, u32, u32, u32, vp, vp]),
    ("navgpu_global_planner_potential_grid", C.c_int, [vp, u32, u32, i32, vp, vp]),
    ("navgpu_navfn_ros_make_plan", C.c_int, [vp, u32, u32, C.POINTER(NavfnRosParams), vp, vp, vp, vp, vp]),
    ("navgpu_navfn_ros_plans", C.c_int, [vp, u32, u32, u32, vp, vp]),
    ("navgpu_navfn_ros_plan_from_potential", C.c_int, [vp, u32, u32, vp, vp, vp]),
    ("navgpu_navfn_ros_compute_potential", C.c_int, [vp, u32, u32, C.POINTER(NavfnRosParams), vp, vp, vp]),
    ("navgpu_navfn_ros_point_potential", C.c_int, [vp, u32, u32, vp, vp, vp, vp]),
    ("navgpu_navfn_ros_valid_point_potential", C.c_int, [vp, u32, u32, vp, vp, vp, vp, vp]),
    ("navgpu_navfn_ros_potential_cloud", C.c_int, [vp, u32, u32, vp, u32, vp, vp]),
    ("navgpu_navfn_path", C.c_int, [vp, u32, vp, u32]),
    ("navgpu_navfn_potential", C.c_int, [vp, u32, vp]),
    ("navgpu_navfn_costarr", C.c_int, [vp, u32, vp]),
    ("navgpu_footprint_radii", C.c_int, [vp, u32, C.POINTER(dbl), C.POINTER(dbl)]),
    ("navgpu_footprint_pad", C.c_int, [vp, u32, dbl]),
    ("navgpu_footprint_from_radius", C.c_int, [dbl, vp]),
    ("navgpu_costmap_export", C.c_int, [vp, u32, u32, u32, u32, u32, vp]),
    ("navgpu_profile_enable", C.c_int, [vp, i32]),
    ("navgpu_profile_select", C.c_int, [vp, u32]),
    ("navgpu_profile_reset", C.c_int, [vp]),
    ("navgpu_profile_read", C.c_int, [vp, i32, C.POINTER(dbl), C.POINTER(C.c_uint64)]),
    ("navgpu_kernel_name", C.c_char_p, [i32]),
    ("navgpu_device_sincos", C.c_int, [i32, vp, u32, vp, vp]),
    ("navgpu_amcl_create", C.c_int, [u32, u32, u32, i32, C.POINTER(vp)]),
    ("navgpu_amcl_destroy", C.c_int, [vp]),
    ("navgpu_amcl_set_map", C.c_int, [vp, u32, u32, vp, u32, u32, dbl, vp, i32, i32, dbl]),
    ("navgpu_amcl_set_map_cells", C.c_int, [vp, u32, u32, vp, u32, u32, dbl, dbl, dbl, i32, dbl]),
    ("navgpu_amcl_set_distance_map", C.c_int, [vp, u32, u32, vp, i32]),
    ("navgpu_amcl_distance_map", C.c_int, [vp, u32, vp]),
    ("navgpu_amcl_laser_configure", C.c_int, [vp, C.POINTER(AmclLaserParams)]),
    ("navgpu_amcl_set_laser_pose", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_set_samples", C.c_int, [vp, u32, u32, vp, vp, vp, vp]),
    ("navgpu_amcl_get_samples", C.c_int, [vp, u32, u32, vp, vp, vp, vp]),
    ("navgpu_amcl_set_filter_state", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_get_filter_state", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_update_sensor", C.c_int, [vp, u32, u32, vp, vp, vp, vp]),
    ("navgpu_amcl_beam_skip_state", C.c_int, [vp, u32, vp, vp, C.POINTER(i32), C.POINTER(i32)]),
    ("navgpu_amcl_resample_configure", C.c_int, [vp, C.POINTER(AmclResampleParams)]),
    ("navgpu_amcl_update_resample", C.c_int, [vp, u32, u32, i32, vp, vp, vp, vp, C.c_uint64, vp]),
    ("navgpu_amcl_get_clusters", C.c_int, [vp, u32, C.POINTER(i32), u32, vp, vp, vp, vp, vp, vp]),
    ("navgpu_amcl_set_kd_leaf_counts", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_get_kd_leaf_counts", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_set_rng_counters", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_get_rng_counters", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_odom_configure", C.c_int, [vp, C.POINTER(AmclOdomParams)]),
    ("navgpu_amcl_update_action", C.c_int, [vp, u32, u32, vp, i32, vp, C.c_uint64, vp]),
    ("navgpu_amcl_init_gaussian", C.c_int, [vp, u32, u32, vp, vp, i32, vp, C.c_uint64, vp]),
    ("navgpu_amcl_init_uniform", C.c_int, [vp, u32, u32, C.POINTER(AmclUniformParams), vp, vp, vp, i32, vp, C.c_uint64, vp, vp]),
    ("navgpu_amcl_node_configure", C.c_int, [vp, C.POINTER(AmclNodeParams)]),
    ("navgpu_amcl_node_laser_received", C.c_int, [vp, u32, u32, vp, vp, C.c_uint64, vp]),
    ("navgpu_amcl_hypotheses", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_node_reset", C.c_int, [vp, u32, u32, i32]),
    ("navgpu_amcl_node_request_nomotion_update", C.c_int, [vp, u32, u32]),
    ("navgpu_amcl_node_integrate_odom", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_node_get_state", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_amcl_node_set_state", C.c_int, [vp, u32, u32, vp]),
    ("navgpu_costmap3d_create", C.c_int, [C.POINTER(Costmap3DDesc), C.POINTER(vp)]),
    ("navgpu_costmap3d_destroy", C.c_int, [vp]),
    ("navgpu_costmap3d_set_origin", C.c_int, [vp, u32, vp]),
    ("navgpu_costmap3d_get_origin", C.c_int, [vp, u32, vp]),
    ("navgpu_costmap3d_set_boxes", C.c_int, [vp, u32, i32, vp, u32, C.POINTER(u32)]),
    ("navgpu_costmap3d_columns_upload", C.c_int, [vp, u32, vp, vp]),
    ("navgpu_costmap3d_columns_download", C.c_int, [vp, u32, vp, vp]),
    ("navgpu_costmap3d_set_mesh", C.c_int, [vp, vp, u32, vp, u32, dbl, C.POINTER(i32)]),
    ("navgpu_costmap3d_query", C.c_int, [vp, u32, vp, vp, i32, vp, vp, vp, dbl, i32, vp, vp]),
    ("navgpu_costmap3d_footprint_costs", C.c_int, [vp, u32, vp, vp, vp, vp]),
    ("navgpu_costmap3d_configure_layers", C.c_int, [vp, vp, u32, i32]),
    ("navgpu_costmap3d_layer_set", C.c_int, [vp, u32, i32, i32]),
    ("navgpu_costmap3d_buffer_clouds", C.c_int, [vp, vp, u32, vp, u32, vp]),
    ("navgpu_costmap3d_set_static_grid", C.c_int, [vp, u32, u32, vp, u32, u32, dbl, dbl, C.POINTER(u32)]),
    ("navgpu_costmap3d_update", C.c_int, [vp, u32, vp, vp, vp]),
    ("navgpu_costmap3d_reset", C.c_int, [vp, u32, vp]),
    ("navgpu_costmap3d_layer2d_download", C.c_int, [vp, u32, u32, u32, u32, u32, vp]),
    ("navgpu_costmap3d_layer2d_update_costs", C.c_int, [vp, u32, vp, vp, C.c_size_t, u32, u32, u32, vp, i32]),
    ("navgpu_costmap3d_layer_columns_download", C.c_int, [vp, u32, u32, vp, vp, vp, vp]),
    ("navgpu_costmap3d_free_columns_download", C.c_int, [vp, u32, vp]),
    ("navgpu_costmap3d_roll", C.c_int, [vp, u32, vp, i32, vp, vp]),
    ("navgpu_costmap3d_reset_bounding_box", C.c_int, [vp, u32, vp, vp, u32]),
    ("navgpu_costmap3d_publisher_configure", C.c_int, [vp, i32]),
    ("navgpu_costmap3d_export", C.c_int, [vp, u32, vp, i32, u32, vp, u32, vp, vp]),
    ("navgpu_costmap3d_layer_update_cells", C.c_int, [vp, u32, vp, vp, i32, vp, u32, vp, u32, vp]),
    ("navgpu_costmap3d_layer_resubscribe", C.c_int, [vp, u32, u32]),
]


def lib():
    """Load libnavgpu.so.  Raises (never falls back) when the HIP extension is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise NavgpuError(f"{path} is missing: build it with navigation_amd.build() / __graft_entry__.build(); "
                          "there is no CPU fallback")
    # (see bench.py / INTEGRATION.md 4: small host-to-device copies through the runtime's copy kernels - its SDMA path stalls ~8 ms once
    # in ~2 500 async copies; a no-op when the HIP runtime of this process has already started or the caller has set the variable)
    os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "2048")
    L = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(L, name)  # AttributeError if the header and the library ever diverge
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def check(rc, what=""):
    if rc < 0:
        L = lib()
        raise NavgpuError(f"{what}: {L.navgpu_strerror(rc).decode()} ({rc}) {L.navgpu_last_error().decode()}")
    return rc
