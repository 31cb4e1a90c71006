"""Fleet: thin Python handle over the navgpu C-ABI (one GPU, N robot instances).

Method names follow the reference interfaces they front:
  update_map            LayeredCostmap::updateMap            (costmap_2d/src/layered_costmap.cpp:79-150)
  add_static_map        StaticLayer::incomingMap             (plugins/static_layer.cpp:167-228)
  set_footprint         LayeredCostmap::setFootprint         (layered_costmap.cpp:164-174)
  set_plan              DWAPlanner::setPlan                  (dwa_local_planner/src/dwa_planner.cpp:204-207)
  set_limits / limits   LocalPlannerUtil::reconfigureCB / getCurrentLimits per robot (base_local_planner/src/local_planner_util.cpp:59-80),
                        MoveSlowAndClear::setRobotSpeed for one robot of a fleet (move_slow_and_clear.cpp:188-214)
  find_best_path        DWAPlanner::updatePlanAndLocalCosts + findBestPath (dwa_planner.cpp:240-371)
  check_trajectory      DWAPlanner::checkTrajectory          (dwa_planner.cpp:213-237)
  check_trajectories    a loop of checkTrajectory calls over robots and velocity probes, one launch
  stage_planner_list / stage_poses_list / planner_cycle_list / results_list  the planner cycle (dwa_planner_ros.cpp:176-247 per robot)
                        for a robot list instead of a contiguous range, one launch of each kernel
  stage_observations_list / obs_stage_list / update_map_list / bounds_list  the costmap update (layered_costmap.cpp:79-150 per robot)
                        for a robot list; a rolling-window fleet takes any list
  footprint_cost        CostmapModel::footprintCost          (base_local_planner/src/costmap_model.cpp:50-142)
  rotate_recovery_step  RotateRecovery::runBehavior, one pass (rotate_recovery/src/rotate_recovery.cpp:105-153)
  carrot_plan           CarrotPlanner::makePlan              (carrot_planner/src/carrot_planner.cpp:116-169)
  voxel_points          costmap_2d_cloud / costmap_2d_markers voxelCallback (costmap_2d/src/costmap_2d_cloud.cpp:85-122)
  voxel_clearing_endpoints  VoxelLayer::raytraceFreespace's clearing_endpoints cloud (plugins/voxel_layer.cpp:286-381)
  obs_buffer / obs_stage  ObservationBuffer::bufferCloud / getObservations behind ObstacleLayer's sensor callbacks
                        (costmap_2d/src/observation_buffer.cpp:111-251, plugins/obstacle_layer.cpp:252-338, 466-496)
  tp_update_plans / tp_score_trajectories  TrajectoryPlanner::updatePlan / scoreTrajectory for a range / a list of robots
                        (base_local_planner/src/trajectory_planner.cpp:474-531)
  tp_update_plans_list / tp_find_best_path_list  updatePlan / findBestPath for a list of robots, one launch set however they lie
  tp_ros_*              TrajectoryPlannerROS::setPlan / computeVelocityCommands / checkTrajectory / isGoalReached for a fleet
                        (base_local_planner/src/trajectory_planner_ros.cpp:283-597)
  trajectory_cloud      DWAPlanner::findBestPath's trajectory_cloud (dwa_planner.cpp:318-348); sample_terms: the breakdown behind it
All compute happens in libnavgpu.so on the GPU; this file only marshals numpy buffers.
"""
import ctypes as C

import numpy as np

from . import _lib as N
from ._lib import (DwaConfig, FleetDesc, InflationParams, NavgpuError, Observation, ObstacleParams, PlanResult,
                   RobotState, check, lib)

_GRID_DTYPE = {N.GRID_MASTER: np.uint8, N.GRID_STATIC: np.uint8, N.GRID_OBSTACLE: np.uint8,
               N.GRID_VOXEL: np.uint32, N.GRID_PATH: np.uint32, N.GRID_GOAL: np.uint32,
               N.GRID_GOAL_FRONT: np.uint32}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Fleet:
    def __init__(self, n_instances, size_x, size_y, resolution, layers=N.LAYER_OBSTACLE | N.LAYER_INFLATION,
                 track_unknown=False, device=0, max_points=1024, max_observations=4, max_plan=256,
                 max_footprint=16, max_sim_steps=64, keep_sample_costs=False, rolling_window=False):
        self.L = lib()
        d = FleetDesc(n_instances, size_x, size_y, resolution, layers, int(track_unknown), device, max_points,
                      max_observations, max_plan, max_footprint, max_sim_steps, int(keep_sample_costs), int(rolling_window))
        self.desc = d
        self.n, self.nx, self.ny, self.res = n_instances, size_x, size_y, resolution
        self.layers = layers
        h = C.c_void_p()
        check(self.L.navgpu_fleet_create(C.byref(d), C.byref(h)), "navgpu_fleet_create")
        self.h = h
        self.cfg = None
        self._footprint = None

    def close(self):
        if getattr(self, "h", None):
            self.L.navgpu_fleet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _range(self, first, count):
        return first, (self.n - first if count is None else count)

    # ---------------------------------------------------------------- grids
    def sync(self):
        check(self.L.navgpu_sync(self.h), "navgpu_sync")

    def set_alloc_limit(self, max_bytes):
        """fault injection for tests: device allocations larger than max_bytes fail from now on (0 = no limit)"""
        check(self.L.navgpu_fleet_set_alloc_limit(self.h, int(max_bytes)), "fleet_set_alloc_limit")

    def origins(self):
        """Current Costmap2D origins (they move with a rolling window)."""
        o = np.zeros((self.n, 2), np.float64)
        check(self.L.navgpu_fleet_get_origin(self.h, 0, self.n, _ptr(o)), "get_origin")
        return o

    def set_origin(self, origins_xy, first=0):
        o = np.ascontiguousarray(origins_xy, np.float64).reshape(-1, 2)
        check(self.L.navgpu_fleet_set_origin(self.h, first, len(o), _ptr(o)), "set_origin")

    def upload(self, grid, cells, first=0):
        a = np.ascontiguousarray(cells, _GRID_DTYPE[grid]).reshape(-1, self.ny, self.nx)
        check(self.L.navgpu_grid_upload(self.h, grid, first, len(a), _ptr(a)), "grid_upload")

    def download(self, grid, first=0, count=None):
        first, count = self._range(first, count)
        out = np.empty((count, self.ny, self.nx), _GRID_DTYPE[grid])
        check(self.L.navgpu_grid_download(self.h, grid, first, count, _ptr(out)), "grid_download")
        return out

    def master(self, first=0, count=None):
        return self.download(N.GRID_MASTER, first, count)

    def export_occupancy(self, instance, x0=0, y0=0, xn=None, yn=None):
        """Costmap2DPublisher's int8 occupancy view of a window of the master grid."""
        xn = self.desc.size_x if xn is None else xn
        yn = self.desc.size_y if yn is None else yn
        out = np.zeros((yn - y0, xn - x0), np.int8)
        check(self.L.navgpu_costmap_export(self.h, instance, x0, y0, xn, yn, _ptr(out)), "costmap_export")
        return out

    def reset(self, grid, first=0, count=None):
        first, count = self._range(first, count)
        check(self.L.navgpu_grid_reset(self.h, grid, first, count), "grid_reset")

    def grid_device(self, grid):
        p, s = C.c_void_p(), C.c_size_t()
        check(self.L.navgpu_grid_device(self.h, grid, C.byref(p), C.byref(s)), "grid_device")
        return p.value, s.value

    def reset_window(self, grid, x0, y0, xn, yn, first=0, count=None):
        """Costmap2D::resetMap(x0, y0, xn, yn) on GRID_MASTER or GRID_OBSTACLE."""
        first, count = self._range(first, count)
        check(self.L.navgpu_grid_reset_window(self.h, grid, first, count, x0, y0, xn, yn), "grid_reset_window")

    def reset_bounding_box(self, boxes, first=0, count=None):
        """CostmapLayer::resetBoundingBox on the obstacle / voxel layer: boxes (count, 4) = min_x, min_y, max_x, max_y (world)."""
        first, count = self._range(first, count)
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(boxes, np.float64).reshape(-1, 4), (count, 4)))
        check(self.L.navgpu_layer_reset_bounding_box(self.h, first, count, _ptr(b)), "layer_reset_bounding_box")

    def set_polygon_cost(self, grid, polygons, value, first=0):
        """Costmap2D::setConvexPolygonCost on GRID_MASTER or GRID_OBSTACLE of robots first ..: one polygon (k, 2) of world points per
        robot (an empty one writes nothing).  Returns a bool per robot: False where a vertex is off the map (nothing written)."""
        polys = [np.ascontiguousarray(p, np.float64).reshape(-1, 2) for p in polygons]
        offsets = np.zeros(len(polys) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(p) for p in polys])
        xy = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((0, 2)))
        ok = np.zeros(len(polys), np.int32)
        check(self.L.navgpu_costmap_set_polygon_cost(self.h, grid, first, len(polys), _ptr(xy) if len(xy) else None, _ptr(offsets),
                                                     int(value), _ptr(ok)), "costmap_set_polygon_cost")
        return [bool(v) for v in ok]

    def clear_costmap_windows(self, poses_xy, size_x, size_y, first=0):
        """MoveBase::clearCostmapWindows on this fleet's master grids: a size_x x size_y window round each robot becomes FREE_SPACE.
        Returns a bool per robot: False where a corner is off the map (nothing cleared, as in the reference)."""
        p = np.ascontiguousarray(np.asarray(poses_xy, np.float64).reshape(-1, 2))
        ok = np.zeros(len(p), np.int32)
        check(self.L.navgpu_move_base_clear_costmap_windows(self.h, first, len(p), _ptr(p), float(size_x), float(size_y), _ptr(ok)),
              "move_base_clear_costmap_windows")
        return [bool(v) for v in ok]

    # ---------------------------------------------------------------- layers
    def add_static_map(self, occupancy, first=0, count=None, track_unknown_space=True, use_maximum=False,
                       trinary_costmap=True, lethal_cost_threshold=100, unknown_cost_value=-1):
        first, count = self._range(first, count)
        occ = np.ascontiguousarray(occupancy, np.int8).reshape(self.ny, self.nx)
        check(self.L.navgpu_static_set_map(self.h, first, count, _ptr(occ), int(track_unknown_space), int(use_maximum),
                                           int(trinary_costmap), lethal_cost_threshold, unknown_cost_value),
              "static_set_map")

    def set_rolling_static_map(self, occupancy, resolution, origin_x, origin_y, track_unknown_space=True, use_maximum=False,
                               trinary_costmap=True, lethal_cost_threshold=100, unknown_cost_value=-1):
        """StaticLayer of a rolling-window fleet: one static map with its own geometry (static_layer.cpp:300-333)."""
        occ = np.ascontiguousarray(occupancy, np.int8)
        sy, sx = occ.shape
        check(self.L.navgpu_static_set_rolling_map(self.h, _ptr(occ), sx, sy, float(resolution), float(origin_x), float(origin_y),
                                                   int(track_unknown_space), int(use_maximum), int(trinary_costmap), lethal_cost_threshold,
                                                   unknown_cost_value), "static_set_rolling_map")

    def set_static_transform(self, basis, origin, first=0, count=None):
        """map_frame <- global_frame per robot: 3x3 basis (row-major) and origin, broadcast when a single one is given."""
        first, count = self._range(first, count)
        b = np.asarray(basis, np.float64).reshape(-1, 9)
        o = np.asarray(origin, np.float64).reshape(-1, 3)
        m = np.ascontiguousarray(np.broadcast_to(np.concatenate([b, o], 1), (count, 12)))
        check(self.L.navgpu_static_set_transform(self.h, first, count, _ptr(m)), "static_set_transform")

    def configure_obstacle(self, enabled=True, footprint_clearing_enabled=True, combination_method=1,
                           max_obstacle_height=2.0, z_voxels=10, origin_z=0.0, z_resolution=0.2,
                           unknown_threshold=15, mark_threshold=0):
        p = ObstacleParams(int(enabled), int(footprint_clearing_enabled), combination_method, z_voxels,
                           max_obstacle_height, origin_z, z_resolution, unknown_threshold, mark_threshold)
        check(self.L.navgpu_obstacle_configure(self.h, C.byref(p)), "obstacle_configure")

    def configure_inflation(self, inflation_radius, cost_scaling_factor, inscribed_radius, enabled=True, priority_queue_order=False):
        """priority_queue_order: reproduce InflationLayer::updateCosts' own priority-queue walk byte for byte (slow)."""
        p = InflationParams(int(enabled), int(priority_queue_order), inflation_radius, cost_scaling_factor, inscribed_radius)
        check(self.L.navgpu_inflation_configure(self.h, C.byref(p)), "inflation_configure")

    def set_footprint(self, xy, first=0, count=None):
        first, count = self._range(first, count)
        fp = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        self._footprint = fp
        check(self.L.navgpu_set_footprint(self.h, first, count, _ptr(fp), len(fp)), "set_footprint")

    # ---------------------------------------------------------------- costmap cycle
    def stage_observations(self, poses, observations, first=0):
        """poses: (count,3).  observations: list of dicts {instance, points(k,3) float32, origin(3),
        obstacle_range, raytrace_range, marking, clearing}."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        count = len(poses)
        obs_arr, allp = self._pack_observations(observations)
        check(self.L.navgpu_costmap_stage(self.h, first, count, _ptr(poses), C.cast(obs_arr, C.c_void_p),
                                          len(observations), _ptr(allp) if len(allp) else None, len(allp)),
              "costmap_stage")

    def stage_observations_raw(self, poses, obs_array, n_obs, points, first=0):
        """Pre-built ctypes Observation array + packed float32 points (bench path, no Python loops)."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        check(self.L.navgpu_costmap_stage(self.h, first, len(poses), _ptr(poses), C.cast(obs_array, C.c_void_p), n_obs,
                                          _ptr(points), len(points)), "costmap_stage")

    def update_map(self, first=0, count=None):
        first, count = self._range(first, count)
        check(self.L.navgpu_costmap_update(self.h, first, count), "costmap_update")

    def bounds(self, first=0, count=None):
        first, count = self._range(first, count)
        b = np.zeros((count, 4), np.int32)
        check(self.L.navgpu_costmap_bounds(self.h, first, count, _ptr(b)), "costmap_bounds")
        return b

    def _pack_observations(self, observations):
        obs_arr = (Observation * max(1, len(observations)))()
        pts = []
        off = 0
        for k, o in enumerate(observations):
            p = np.ascontiguousarray(o["points"], np.float32).reshape(-1, 3)
            flags = (N.OBS_MARKING if o.get("marking", True) else 0) | (N.OBS_CLEARING if o.get("clearing", True) else 0)
            org = o.get("origin", (0.0, 0.0, 1.0))
            obs_arr[k] = Observation(o["instance"], off, len(p), flags, org[0], org[1], org[2],
                                     o.get("obstacle_range", 2.5), o.get("raytrace_range", 3.0))
            pts.append(p)
            off += len(p)
        allp = np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)
        return obs_arr, np.ascontiguousarray(allp, np.float32)

    def stage_observations_list(self, instances, poses, observations):
        """stage_observations for the robots `instances` (strictly increasing): poses[k] belongs to instances[k]; an observation's
        `instance` stays a fleet index and must be in the list.  One packed upload, one scatter launch."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        if len(poses) != len(inst):
            raise ValueError("stage_observations_list: one pose per listed robot")
        obs_arr, allp = self._pack_observations(observations)
        check(self.L.navgpu_costmap_stage_list(self.h, len(inst), _ptr(inst), _ptr(poses), C.cast(obs_arr, C.c_void_p), len(observations),
                                               _ptr(allp) if len(allp) else None, len(allp)), "costmap_stage_list")

    def stage_observations_list_raw(self, instances, poses, obs_array, n_obs, points):
        """Pre-built ctypes Observation array + packed float32 points (no Python loops on the per-cycle path)."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        check(self.L.navgpu_costmap_stage_list(self.h, len(inst), _ptr(inst), _ptr(poses), C.cast(obs_array, C.c_void_p), n_obs,
                                               _ptr(points), len(points)), "costmap_stage_list")

    def obs_stage_list(self, instances, poses, now_ns, want_current=True):
        """obs_stage for the robots `instances`.  Returns isCurrent per listed robot (bool array)."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        if len(poses) != len(inst):
            raise ValueError("obs_stage_list: one pose per listed robot")
        cur = np.zeros(len(inst), np.int32)
        check(self.L.navgpu_obsbuf_stage_list(self.h, len(inst), _ptr(inst), _ptr(poses), int(now_ns), _ptr(cur) if want_current else None),
              "obsbuf_stage_list")
        return cur.astype(bool)

    def update_map_list(self, instances):
        """update_map for the robots `instances`: one launch of each kernel, the robots outside the list untouched."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        check(self.L.navgpu_costmap_update_list(self.h, len(inst), _ptr(inst)), "costmap_update_list")

    def bounds_list(self, instances):
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        b = np.zeros((len(inst), 4), np.int32)
        check(self.L.navgpu_costmap_bounds_list(self.h, len(inst), _ptr(inst), _ptr(b)), "costmap_bounds_list")
        return b

    def inflate(self, boxes=None, first=0, count=None):
        first, count = self._range(first, count)
        if boxes is None:
            check(self.L.navgpu_inflate(self.h, first, count, None), "inflate")
        else:
            b = np.ascontiguousarray(boxes, np.int32).reshape(count, 4)
            check(self.L.navgpu_inflate(self.h, first, count, _ptr(b)), "inflate")

    def obstacle_update_bounds(self, bounds, first=0):
        b = np.ascontiguousarray(bounds, np.float64).reshape(-1, 4).copy()
        check(self.L.navgpu_obstacle_update_bounds(self.h, first, len(b), _ptr(b)), "obstacle_update_bounds")
        return b

    def obstacle_update_costs(self, boxes, first=0):
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        check(self.L.navgpu_obstacle_update_costs(self.h, first, len(b), _ptr(b)), "obstacle_update_costs")

    # ---------------------------------------------------------------- ObservationBuffer on the device
    def obs_configure(self, sources, slots, max_cloud_points):
        """sources: ObsSourceParams, or dicts of its fields, one per entry of observation_sources."""
        arr = (N.ObsSourceParams * len(sources))(*[s if isinstance(s, N.ObsSourceParams) else N.ObsSourceParams(**s) for s in sources])
        check(self.L.navgpu_obsbuf_configure(self.h, C.cast(arr, C.c_void_p), len(sources), int(slots), int(max_cloud_points)), "obsbuf_configure")

    @staticmethod
    def pack_clouds(clouds):
        """The arguments of navgpu_obsbuf_buffer from a list of dicts {instance, source, stamp_ns, origin(3), transform(12):
        basis row-major then origin} with either points (k, 3) float32, or ranges (k,) float32 and angle_min, angle_increment,
        range_min, range_max: (Cloud array, packed points, packed ranges)."""
        arr = (N.Cloud * max(1, len(clouds)))()
        pts, rng = [], []
        n_pts = n_rng = 0
        for k, c in enumerate(clouds):
            a = arr[k]
            a.instance, a.source, a.stamp_ns = c["instance"], c.get("source", 0), int(c["stamp_ns"])
            a.origin[:] = [float(v) for v in c.get("origin", (0.0, 0.0, 0.0))]
            a.transform[:] = [float(v) for v in np.asarray(c.get("transform", (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)), np.float64).ravel()]
            if "ranges" in c:
                r = np.ascontiguousarray(c["ranges"], np.float32).ravel()
                a.kind, a.first, a.n = N.CLOUD_SCAN, n_rng, len(r)
                a.angle_min, a.angle_increment, a.range_min, a.range_max = (float(c[k]) for k in ("angle_min", "angle_increment", "range_min", "range_max"))
                rng.append(r)
                n_rng += len(r)
            else:
                p = np.ascontiguousarray(c["points"], np.float32).reshape(-1, 3)
                a.kind, a.first, a.n = N.CLOUD_XYZ, n_pts, len(p)
                pts.append(p)
                n_pts += len(p)
        points = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 3), np.float32), np.float32)
        ranges = np.ascontiguousarray(np.concatenate(rng) if rng else np.zeros(0, np.float32), np.float32)
        return arr, points, ranges

    def obs_buffer(self, clouds, now_ns):
        """ObservationBuffer::bufferCloud for every cloud / scan of `clouds` (see pack_clouds), in order."""
        arr, points, ranges = self.pack_clouds(clouds)
        self.obs_buffer_raw(arr, len(clouds), points, ranges, now_ns)

    def obs_buffer_raw(self, cloud_array, n_clouds, points, ranges, now_ns):
        """Pre-built ctypes Cloud array + packed float32 points / ranges (no Python loops on the per-cycle path)."""
        check(self.L.navgpu_obsbuf_buffer(self.h, C.cast(cloud_array, C.c_void_p), n_clouds, _ptr(points) if len(points) else None, len(points),
                                          _ptr(ranges) if len(ranges) else None, len(ranges), int(now_ns)), "obsbuf_buffer")

    def obs_stage(self, poses, now_ns, first=0, want_current=True):
        """getMarkingObservations + getClearingObservations + the staging of the cycle.  Returns isCurrent per robot (bool array)."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        cur = np.zeros(len(poses), np.int32)
        check(self.L.navgpu_obsbuf_stage(self.h, first, len(poses), _ptr(poses), int(now_ns), _ptr(cur) if want_current else None), "obsbuf_stage")
        return cur.astype(bool)

    def obs_observations(self, instance, now_ns=0):
        """What obs_stage would hand over for one robot: a list of dicts {flags, origin, obstacle_range, raytrace_range, points (k, 3)}."""
        max_obs = max(1, self.desc.max_observations)
        obs = (Observation * max_obs)()
        pts = np.zeros((max(1, self.obs_status(instance, 1)[0].points), 3), np.float32)
        n_pts = C.c_uint32()
        n = check(self.L.navgpu_obsbuf_observations(self.h, instance, int(now_ns), C.cast(obs, C.c_void_p), max_obs, _ptr(pts), len(pts), C.byref(n_pts)),
                  "obsbuf_observations")
        return [dict(flags=o.flags, origin=(o.origin_x, o.origin_y, o.origin_z), obstacle_range=o.obstacle_range, raytrace_range=o.raytrace_range,
                     points=pts[o.first_point:o.first_point + o.n_points].copy()) for o in obs[:n]]

    def obs_status(self, first=0, count=None):
        first, count = self._range(first, count)
        out = (N.ObsBufRobotStatus * count)()
        check(self.L.navgpu_obsbuf_status(self.h, first, count, C.cast(out, C.c_void_p)), "obsbuf_status")
        return list(out)

    def obs_set_global_frame(self, transforms12, first=0, count=None):
        """ObservationBuffer::setGlobalFrame with the looked-up new_global <- global transform, one per robot or one for all."""
        first, count = self._range(first, count)
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(transforms12, np.float64).reshape(-1, 12), (count, 12)))
        check(self.L.navgpu_obsbuf_set_global_frame(self.h, first, count, _ptr(m)), "obsbuf_set_global_frame")

    def obs_reset_last_updated(self, now_ns, first=0, count=None):
        first, count = self._range(first, count)
        check(self.L.navgpu_obsbuf_reset_last_updated(self.h, first, count, int(now_ns)), "obsbuf_reset_last_updated")

    # ---------------------------------------------------------------- planner
    def configure_planner(self, cfg):
        self.cfg = cfg
        check(self.L.navgpu_planner_configure(self.h, C.byref(cfg)), "planner_configure")

    @staticmethod
    def _limit_records(limits):
        """A list of dicts, a structured array or a (RobotLimits * n) array as a ctypes array; raises before any library call when a
        record misses a field, names an unknown one or holds something that is no number."""
        if isinstance(limits, C.Array) and getattr(limits, "_type_", None) is N.RobotLimits:
            return limits
        names = N.RobotLimits.FIELDS
        if isinstance(limits, np.ndarray):
            if limits.dtype.names is None:
                raise ValueError("set_limits: an array of limits must be a structured array with the fields of navgpu_robot_limits")
            rows = [{n: r[n] for n in limits.dtype.names} for r in np.atleast_1d(limits)]
        elif isinstance(limits, dict):
            rows = [limits]
        else:
            rows = list(limits)
        if not rows:
            raise ValueError("set_limits: no record")
        out = (N.RobotLimits * len(rows))()
        for k, r in enumerate(rows):
            if not isinstance(r, dict):
                raise ValueError(f"set_limits: record {k} is not a dict")
            missing, unknown = [n for n in names if n not in r], [n for n in r if n not in names and n != "reserved"]
            if missing or unknown:
                raise ValueError(f"set_limits: record {k}: missing fields {missing}, unknown fields {unknown}")
            for n in names:
                v = r[n]
                if isinstance(v, (bool, np.bool_)) and n != "prune_plan" or not isinstance(v, (int, float, bool, np.integer, np.floating, np.bool_)):
                    raise ValueError(f"set_limits: record {k}: {n} = {v!r} is not a number")
                setattr(out[k], n, int(v) if n == "prune_plan" else float(v))
        return out

    def set_limits(self, limits, first=0):
        """LocalPlannerUtil::reconfigureCB / MoveSlowAndClear::setRobotSpeed for the robots first, first + 1, ...: one record of
        LocalPlannerLimits each (a list of dicts, or a structured array, with the fields of navgpu_robot_limits).  The robots'
        next staged cycle or probe runs on them; the others stay as they were."""
        rec = self._limit_records(limits)
        check(self.L.navgpu_planner_set_limits(self.h, first, len(rec), C.cast(rec, C.c_void_p)), "planner_set_limits")

    def limits(self, first=0, count=None):
        """LocalPlannerUtil::getCurrentLimits per robot: a list of dicts with the fields of navgpu_robot_limits."""
        first, count = self._range(first, count)
        rec = (N.RobotLimits * count)()
        check(self.L.navgpu_planner_get_limits(self.h, first, count, C.cast(rec, C.c_void_p)), "planner_get_limits")
        return [r.as_dict() for r in rec]

    def set_plan(self, first=0, count=None):
        first, count = self._range(first, count)
        check(self.L.navgpu_planner_set_plan(self.h, first, count), "planner_set_plan")

    def stage_planner(self, pos, vel, plans, first=0):
        """pos, vel: (count,3) float32.  plans: (count, K, 2) array or list of (k_i,2) arrays."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
        count = len(pos)
        if isinstance(plans, np.ndarray) and plans.ndim == 3:
            packed = np.ascontiguousarray(plans, np.float64).reshape(-1, 2)
            counts = [plans.shape[1]] * count
        else:
            counts = [len(p) for p in plans]
            packed = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in plans]))
        states = (RobotState * count)()
        off = 0
        for i in range(count):
            states[i].pos[:] = pos[i].tolist()
            states[i].vel[:] = vel[i].tolist()
            states[i].plan_first = off
            states[i].plan_count = counts[i]
            off += counts[i]
        check(self.L.navgpu_planner_stage(self.h, first, count, C.cast(states, C.c_void_p), _ptr(packed), len(packed)),
              "planner_stage")

    def stage_planner_raw(self, states, n, packed_plans, first=0):
        check(self.L.navgpu_planner_stage(self.h, first, n, C.cast(states, C.c_void_p), _ptr(packed_plans),
                                          len(packed_plans)), "planner_stage")

    def stage_poses(self, pos, vel, first=0):
        """A control cycle whose plan is unchanged: pose + velocity only (pos, vel: (count, 3) float32, C-contiguous)."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
        check(self.L.navgpu_planner_stage_poses(self.h, first, len(pos), _ptr(pos), _ptr(vel)), "planner_stage_poses")

    def wavefront_boxes(self, first=0, count=None):
        """Cell boxes (x0, x1, y0, y1, inclusive) the last cycle's bounded wavefronts settled, [count, 4]."""
        first, count = self._range(first, count)
        out = np.zeros((count, 4), np.int32)
        check(self.L.navgpu_planner_wavefront_boxes(self.h, first, count, _ptr(out)), "wavefront_boxes")
        return out

    MAP_GRID_CRITICS = {"path": 0, "goal": 1, "goal_front": 2, "alignment": 3}
    AGGREGATIONS = {"last": 0, "sum": 1, "product": 2}

    def set_map_grid_options(self, critic, aggregation="last", yshift=0.0):
        """MapGridCostFunction's aggregationType / yshift of one of DWAPlanner's four map-grid critics."""
        check(self.L.navgpu_planner_set_map_grid_options(self.h, self.MAP_GRID_CRITICS[critic], self.AGGREGATIONS[aggregation], float(yshift)),
              "set_map_grid_options")

    def set_bounded_map_grids(self, enable):
        """navgpu_planner_set_bounded_map_grids: wavefronts stop once the robot's box is settled (default on)."""
        check(self.L.navgpu_planner_set_bounded_map_grids(self.h, 1 if enable else 0), "set_bounded_map_grids")

    def set_seed_lists(self, enable):
        """navgpu_planner_set_seed_lists: a cycle's k_samples turns the plans into the wavefronts' seed cells (default on)."""
        check(self.L.navgpu_planner_set_seed_lists(self.h, 1 if enable else 0), "set_seed_lists")

    def set_split_prep(self, enable):
        """navgpu_planner_set_split_prep: the grid-free part of the scoring image is built inside the wavefront launch (default on)."""
        check(self.L.navgpu_planner_set_split_prep(self.h, 1 if enable else 0), "set_split_prep")

    def set_seed_list_capacity(self, cells):
        """navgpu_planner_set_seed_list_capacity (test hook): a (robot, grid) with more seed cells walks the plan itself."""
        check(self.L.navgpu_planner_set_seed_list_capacity(self.h, int(cells)), "set_seed_list_capacity")

    def seed_list_counts(self, first=0, count=None):
        """Seed cells listed for the path / goal / goal_front wavefronts, [count, 3]; 0xFFFFFFFF = no list."""
        first, count = self._range(first, count)
        out = np.zeros((count, 3), np.uint32)
        check(self.L.navgpu_planner_seed_list_counts(self.h, first, count, _ptr(out)), "seed_list_counts")
        return out

    def wavefront_levels(self, first=0, count=None):
        """Levels the last cycle's path / goal / goal_front wavefronts ran, [count, 3]."""
        first, count = self._range(first, count)
        out = np.zeros((count, 3), np.uint32)
        check(self.L.navgpu_planner_wavefront_levels(self.h, first, count, _ptr(out)), "wavefront_levels")
        return out

    def planner_cycle(self, first=0, count=None):
        first, count = self._range(first, count)
        check(self.L.navgpu_planner_cycle(self.h, first, count), "planner_cycle")

    def results(self, first=0, count=None):
        first, count = self._range(first, count)
        r = (PlanResult * count)()
        check(self.L.navgpu_planner_results(self.h, first, count, C.cast(r, C.c_void_p)), "planner_results")
        return list(r)

    def results_into(self, buf, first=0):
        """Same as results() but into a caller-owned (PlanResult * count) array: no Python allocation on
        the per-cycle path (a list of 256 fresh ctypes objects per call makes the interpreter's garbage
        collector the slowest part of a cycle once a large package such as torch is imported)."""
        check(self.L.navgpu_planner_results(self.h, first, len(buf), C.cast(buf, C.c_void_p)), "planner_results")
        return buf

    def set_cycles_in_flight(self, cycles):
        """navgpu_planner_set_cycles_in_flight: 2 = cycle k + 1 is handed over and queued while cycle k runs."""
        check(self.L.navgpu_planner_set_cycles_in_flight(self.h, int(cycles)), "set_cycles_in_flight")

    def results_previous_into(self, buf, first=0):
        """Results of the cycle before the latest queued one (two cycles in flight), into a (PlanResult * count) array."""
        check(self.L.navgpu_planner_results_previous(self.h, first, len(buf), C.cast(buf, C.c_void_p)), "planner_results_previous")
        return buf

    def find_best_path(self, pos, vel, plans, first=0):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self.stage_planner(pos, vel, plans, first)
        self.planner_cycle(first, len(pos))
        return self.results(first, len(pos))

    def trajectory(self, instance):
        cap = self.desc.max_sim_steps
        out = np.zeros((cap, 3), np.float64)
        n = check(self.L.navgpu_planner_trajectory(self.h, instance, _ptr(out), cap), "planner_trajectory")
        return out[:n].copy()

    def samples(self, instance):
        cfg = self.cfg
        cap = (max(cfg.vx_samples, 2) + 1) * (max(cfg.vy_samples, 2) + 1) * (max(cfg.vth_samples, 2) + 1)
        cost = np.zeros(cap, np.float64)
        status = np.zeros(cap, np.int32)
        vel = np.zeros((cap, 3), np.float32)
        n = check(self.L.navgpu_planner_samples(self.h, instance, _ptr(cost), _ptr(status), _ptr(vel), cap),
                  "planner_samples")
        return cost[:n].copy(), status[:n].copy(), vel[:n].copy()

    def check_trajectory(self, instance, vel_samples):
        v = np.ascontiguousarray(vel_samples, np.float32)
        ok = C.c_int32()
        check(self.L.navgpu_planner_check_trajectory(self.h, instance, _ptr(v), C.byref(ok)), "check_trajectory")
        return bool(ok.value)

    def check_trajectories(self, instances, probes, offsets=None):
        """DWAPlanner::checkTrajectory for a list of robots (strictly increasing indices), each with a run of velocity probes,
        in one launch.  probes: a list of (n_k, 3) arrays, one per robot, or - with offsets (len(instances) + 1, from 0) - one
        flat (total, 3) array.  Returns (ok, costs): bool and float64 per probe, in probe order; costs as scoreTrajectory
        returns them (the weighted sum, or the first failing critic's code)."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        if offsets is None:
            runs = [np.asarray(p, np.float32).reshape(-1, 3) for p in probes]
            off = np.zeros(len(runs) + 1, np.uint32)
            off[1:] = np.cumsum([len(r) for r in runs])
            vel = np.concatenate(runs) if runs else np.zeros((0, 3), np.float32)
        else:
            off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
            vel = np.asarray(probes, np.float32).reshape(-1, 3)
        if len(off) != len(inst) + 1 or (len(off) and int(off[-1]) != len(vel)):
            raise ValueError("check_trajectories: one run of probes per robot (offsets: len(instances) + 1 entries ending at the probe count)")
        vel = np.ascontiguousarray(vel, np.float32)
        ok = np.zeros(max(len(vel), 1), np.int32)
        costs = np.zeros(max(len(vel), 1), np.float64)
        check(self.L.navgpu_planner_check_trajectories(self.h, len(inst), _ptr(inst), _ptr(off), _ptr(vel), _ptr(ok), _ptr(costs)),
              "check_trajectories")
        return ok[:len(vel)].astype(bool), costs[:len(vel)].copy()

    # ---- the planner cycle for a robot list (strictly increasing indices): one launch of each kernel whatever the list looks like
    def stage_planner_list(self, instances, pos, vel, plans):
        """stage_planner for the listed robots; pos, vel, plans are indexed by list position."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
        if len(pos) != len(inst) or len(vel) != len(inst) or len(plans) != len(inst):
            raise ValueError("stage_planner_list: one pose, velocity and plan per listed robot")
        counts = [len(p) for p in plans]
        packed = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in plans])) if counts else np.zeros((0, 2))
        states = (RobotState * max(len(inst), 1))()
        off = 0
        for k in range(len(inst)):
            states[k].pos[:] = pos[k].tolist()
            states[k].vel[:] = vel[k].tolist()
            states[k].plan_first = off
            states[k].plan_count = counts[k]
            off += counts[k]
        check(self.L.navgpu_planner_stage_list(self.h, len(inst), _ptr(inst), C.cast(states, C.c_void_p), _ptr(packed), len(packed)),
              "planner_stage_list")

    def stage_poses_list(self, instances, pos, vel):
        """stage_poses for the listed robots (plans unchanged); pos, vel: one row per listed robot."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
        if len(pos) != len(inst) or len(vel) != len(inst):
            raise ValueError("stage_poses_list: one pose and velocity per listed robot")
        check(self.L.navgpu_planner_stage_poses_list(self.h, len(inst), _ptr(inst), _ptr(pos), _ptr(vel)), "planner_stage_poses_list")

    def planner_cycle_list(self, instances):
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        check(self.L.navgpu_planner_cycle_list(self.h, len(inst), _ptr(inst)), "planner_cycle_list")

    def results_list(self, instances):
        """The results of the listed robots, in list order."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        r = (PlanResult * max(len(inst), 1))()
        check(self.L.navgpu_planner_results_list(self.h, len(inst), _ptr(inst), C.cast(r, C.c_void_p)), "planner_results_list")
        return list(r)[:len(inst)]

    def cost_cloud(self, instance):
        """MapGridVisualizer's cost cloud of one robot: (n, 7) float32 x, y, z, path, goal, occ, total."""
        cap = self.desc.size_x * self.desc.size_y
        buf = np.zeros((cap, 7), np.float32)
        n = check(self.L.navgpu_planner_cost_cloud(self.h, instance, _ptr(buf), cap), "cost_cloud")
        return buf[:n].copy()

    def set_trajectory_cloud(self, enable=True, first=0, count=None):
        """publish_traj_pc per robot: an enabled robot's cycles keep the per-sample critic terms (at most 16 robots)."""
        first, count = self._range(first, count)
        check(self.L.navgpu_planner_set_trajectory_cloud(self.h, first, count, 1 if enable else 0), "set_trajectory_cloud")

    def trajectory_cloud(self, instance, reference_costs=True):
        """DWAPlanner's trajectory_cloud of one enabled robot's last cycle: (n, 7) float32 x, y, z, path_cost (= theta),
        goal_cost, occ_cost, total_cost; every point of every explored trajectory with a cost >= 0, in slot order.
        reference_costs: the reference's early-out costs, else every slot's full sum."""
        ref = 1 if reference_costs else 0
        n = check(self.L.navgpu_planner_trajectory_cloud(self.h, instance, ref, None, 0), "trajectory_cloud")
        buf = np.zeros((n, 7), np.float32)
        if n:
            check(self.L.navgpu_planner_trajectory_cloud(self.h, instance, ref, _ptr(buf), n), "trajectory_cloud")
        return buf

    SAMPLE_TERMS_DTYPE = np.dtype([("critic", np.float64, 5), ("cost_full", np.float64), ("cost_ref", np.float64), ("first_fail", np.int32),
                                   ("status", np.int32), ("n_points", np.int32), ("member", np.int32), ("point_offset", np.uint32),
                                   ("reserved", np.uint32)])

    def sample_terms(self, instance):
        """Per-slot breakdown behind trajectory_cloud: a structured array (navgpu_sample_terms) in slot order."""
        n = check(self.L.navgpu_planner_sample_terms(self.h, instance, None, 0), "sample_terms")
        out = np.zeros(n, self.SAMPLE_TERMS_DTYPE)
        if n:
            check(self.L.navgpu_planner_sample_terms(self.h, instance, _ptr(out), n), "sample_terms")
        return out

    def oscillation(self, first=0, count=None):
        first, count = self._range(first, count)
        flags = np.zeros(count, np.uint32)
        prev = np.zeros((count, 3), np.float32)
        check(self.L.navgpu_planner_get_oscillation(self.h, first, count, _ptr(flags), _ptr(prev)), "get_oscillation")
        return flags, prev

    def set_oscillation(self, flags, prev=None, first=0):
        flags = np.ascontiguousarray(flags, np.uint32)
        p = None if prev is None else _ptr(np.ascontiguousarray(prev, np.float32))
        check(self.L.navgpu_planner_set_oscillation(self.h, first, len(flags), _ptr(flags), p), "set_oscillation")

    # ---------------------------------------------------------------- DWAPlannerROS control cycle
    def configure_local_planner(self, **limits):
        """LocalPlannerLimits + LatchedStopRotateController parameters (navgpu_local_limits)."""
        lim = N.LocalLimits(**limits)
        check(self.L.navgpu_local_planner_configure(self.h, C.byref(lim)), "local_planner_configure")

    def set_global_plan(self, instance, plan_xyyaw, plan_to_global=None):
        """DWAPlannerROS::setPlan for one robot."""
        plan = np.ascontiguousarray(plan_xyyaw, np.float64).reshape(-1, 3)
        T = None if plan_to_global is None else _ptr(np.ascontiguousarray(plan_to_global, np.float64))
        check(self.L.navgpu_local_planner_set_plan(self.h, instance, _ptr(plan), len(plan), T), "local_planner_set_plan")

    def global_plan(self, instance):
        n = check(self.L.navgpu_local_planner_get_plan(self.h, instance, None, 0), "local_planner_get_plan")
        out = np.zeros((n, 3))
        if n:
            check(self.L.navgpu_local_planner_get_plan(self.h, instance, _ptr(out), n), "local_planner_get_plan")
        return out

    def reserve_global_plans(self, max_global_plan):
        """Allocates (or resizes) the device store of global plans: n_instances x max_global_plan poses."""
        check(self.L.navgpu_local_planner_reserve_plans(self.h, int(max_global_plan)), "local_planner_reserve_plans")

    def set_global_plans(self, plans_xyyaw, plans_to_global=None, first=0):
        """DWAPlannerROS::setPlan for robots first .. first + len(plans) - 1 in one upload; the plans stay on the device.
        plans_to_global: None, or one (x, y, yaw) per plan (all plans then carry a transform)."""
        plans = [np.ascontiguousarray(p, np.float64).reshape(-1, 3) for p in plans_xyyaw]
        offsets = np.zeros(len(plans) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(p) for p in plans])
        poses = np.ascontiguousarray(np.concatenate(plans) if plans else np.zeros((0, 3)))
        T = None if plans_to_global is None else np.ascontiguousarray(plans_to_global, np.float64).reshape(len(plans), 3)
        check(self.L.navgpu_local_planner_set_plans(self.h, first, len(plans), _ptr(poses) if len(poses) else None, _ptr(offsets),
                                                    None if T is None else _ptr(T)), "local_planner_set_plans")

    def adopt_global_plans(self, navfn, family, count=None, first=0, nav_first=0, plans_to_global=None):
        """The plans nav_first .. of a NavFn batch's last make_plan (family: PLAN_FAMILY_GLOBAL_PLANNER / _NAVFN_ROS) become the
        plans of robots first ..; nothing leaves the device.  Returns a bool per robot: adopted (False: the plan was not made or is
        too long; the robot keeps its previous plan).  On NAVGPU_ERR_CAPACITY the others were adopted first: the NavgpuError raised
        carries that list as `.adopted`."""
        count = navfn.n - nav_first if count is None else count
        T = None if plans_to_global is None else np.ascontiguousarray(plans_to_global, np.float64).reshape(count, 3)
        adopted = np.zeros(count, np.int32)
        rc = self.L.navgpu_local_planner_adopt_plans(self.h, first, navfn.h, nav_first, count, int(family), None if T is None else _ptr(T),
                                                     _ptr(adopted))
        try:
            check(rc, "local_planner_adopt_plans")
        except NavgpuError as e:
            e.adopted = [bool(v) for v in adopted] if rc == -4 else None  # NAVGPU_ERR_CAPACITY: who was adopted before the error
            raise
        return [bool(v) for v in adopted]

    def handover_global_plans(self, navfn, family, positions_xy, now_ns, persistence_timeout_ns=10_000_000_000, count=None, first=0,
                              nav_first=0, plans_to_global=None):
        """move_base's handover of a NavFn batch's plans with MoveBase::preferPrevPlan's persistence policy, decided on the device:
        adopt_global_plans' arguments, the robots' positions in their plans' frame (count, 2) and the time.  Returns a list of
        HandoverRecord.  On NAVGPU_ERR_CAPACITY the others were handled first: the NavgpuError raised carries the list as `.records`."""
        count = navfn.n - nav_first if count is None else count
        T = None if plans_to_global is None else np.ascontiguousarray(plans_to_global, np.float64).reshape(count, 3)
        pos = np.ascontiguousarray(np.asarray(positions_xy, np.float64).reshape(count, 2))
        out = (N.HandoverRecord * count)()
        rc = self.L.navgpu_move_base_handover_plans(self.h, first, navfn.h, nav_first, count, int(family), None if T is None else _ptr(T),
                                                    _ptr(pos), int(now_ns), int(persistence_timeout_ns), out)
        try:
            check(rc, "move_base_handover_plans")
        except NavgpuError as e:
            e.records = list(out) if rc == -4 else None
            raise
        return list(out)

    def reset_plan_persistence(self, first=0, count=None):
        """persistence_end_ = PERSISTENCE_INITIAL (a new goal)."""
        first, count = self._range(first, count)
        check(self.L.navgpu_move_base_reset_persistence(self.h, first, count), "move_base_reset_persistence")

    def plan_persistence(self, first=0, count=None):
        first, count = self._range(first, count)
        out = np.zeros(count, np.int64)
        check(self.L.navgpu_move_base_get_persistence(self.h, first, count, _ptr(out)), "move_base_get_persistence")
        return out

    def set_plan_persistence(self, persistence_end_ns, first=0):
        a = np.ascontiguousarray(persistence_end_ns, np.int64).reshape(-1)
        check(self.L.navgpu_move_base_set_persistence(self.h, first, len(a), _ptr(a)), "move_base_set_persistence")

    def local_plan(self, instance):
        """The transformed, pruned plan of the robot's last cycle, (m, 3)."""
        n = check(self.L.navgpu_local_planner_local_plan(self.h, instance, None, 0), "local_planner_local_plan")
        out = np.zeros((n, 3))
        if n:
            check(self.L.navgpu_local_planner_local_plan(self.h, instance, _ptr(out), n), "local_planner_local_plan")
        return out

    def local_windows(self, first=0, count=None):
        """navgpu_local_window of the last cycle per robot -> list of LocalWindow."""
        count = self.n - first if count is None else count
        out = (N.LocalWindow * count)()
        check(self.L.navgpu_local_planner_windows(self.h, first, count, out), "local_planner_windows")
        return list(out)

    def _robot_inputs(self, poses, odom_vels, have_pose):
        poses = np.asarray(poses, np.float64).reshape(-1, 3)
        vels = np.asarray(odom_vels, np.float64).reshape(-1, 3)
        arr = (N.RobotInput * len(poses))()
        for k in range(len(poses)):
            arr[k].pose[:] = [float(v) for v in poses[k]]
            arr[k].odom_vel[:] = [float(v) for v in vels[k]]
            arr[k].have_pose = 1 if have_pose is None else int(bool(have_pose[k]))
        return arr

    def compute_velocity_commands(self, poses, odom_vels, first=0, have_pose=None):
        """DWAPlannerROS::computeVelocityCommands for len(poses) robots -> list of CmdResult."""
        arr = self._robot_inputs(poses, odom_vels, have_pose)
        out = (N.CmdResult * len(arr))()
        check(self.L.navgpu_local_planner_compute_velocity_commands(self.h, first, len(arr), arr, out), "compute_velocity_commands")
        return list(out)

    def is_goal_reached(self, poses, odom_vels, first=0, have_pose=None):
        arr = self._robot_inputs(poses, odom_vels, have_pose)
        out = (C.c_int32 * len(arr))()
        check(self.L.navgpu_local_planner_is_goal_reached(self.h, first, len(arr), arr, out), "is_goal_reached")
        return [bool(v) for v in out]

    # ---------------------------------------------------------------- legacy TrajectoryPlanner
    def configure_trajectory_planner(self, cfg):
        check(self.L.navgpu_tp_configure(self.h, C.byref(cfg)), "tp_configure")

    def tp_update_plan(self, instance, plan_xy, compute_dists=False):
        plan = np.ascontiguousarray(plan_xy, np.float64).reshape(-1, 2)
        check(self.L.navgpu_tp_update_plan(self.h, instance, _ptr(plan) if len(plan) else None, len(plan), int(compute_dists)),
              "tp_update_plan")

    def tp_find_best_path(self, pos, vel, first=0):
        """TrajectoryPlanner::findBestPath for len(pos) robots -> list of TpResult."""
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        vel = np.asarray(vel, np.float32).reshape(-1, 3)
        st = (N.RobotState * len(pos))()
        for k in range(len(pos)):
            st[k].pos[:] = [float(v) for v in pos[k]]
            st[k].vel[:] = [float(v) for v in vel[k]]
        out = (N.TpResult * len(pos))()
        check(self.L.navgpu_tp_find_best_path(self.h, first, len(pos), st, out), "tp_find_best_path")
        return list(out)

    def tp_trajectory(self, instance):
        buf = np.zeros((self.desc.max_sim_steps, 3))
        n = check(self.L.navgpu_tp_trajectory(self.h, instance, _ptr(buf), len(buf)), "tp_trajectory")
        return buf[:n].copy()

    def tp_samples(self, instance):
        n = check(self.L.navgpu_tp_samples(self.h, instance, None, 0), "tp_samples")
        arr = (N.TpSample * max(n, 1))()
        check(self.L.navgpu_tp_samples(self.h, instance, arr, n), "tp_samples")
        return [(a.vx, a.vy, a.vtheta, a.cost, a.n_points) for a in arr[:n]]

    def tp_score_trajectory(self, instance, pose, vel, vel_samples):
        cost = C.c_double()
        a, b, c3 = (np.ascontiguousarray(v, np.float64) for v in (pose, vel, vel_samples))
        check(self.L.navgpu_tp_score_trajectory(self.h, instance, _ptr(a), _ptr(b), _ptr(c3), C.byref(cost)), "tp_score_trajectory")
        return cost.value

    def tp_state(self, first=0, count=None):
        first, count = self._range(first, count)
        arr = (N.TpState * count)()
        check(self.L.navgpu_tp_get_state(self.h, first, count, arr), "tp_get_state")
        return list(arr)

    def tp_set_state(self, states, first=0):
        arr = (N.TpState * len(states))(*states)
        check(self.L.navgpu_tp_set_state(self.h, first, len(states), arr), "tp_set_state")

    def tp_update_plans(self, plans_xy, compute_dists=False, first=0):
        """TrajectoryPlanner::updatePlan for robots first .. first + len(plans_xy) - 1: one upload, one wavefront launch, one wait."""
        plans = [np.ascontiguousarray(p, np.float64).reshape(-1, 2) for p in plans_xy]
        offsets = np.zeros(len(plans) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(p) for p in plans])
        xy = np.ascontiguousarray(np.concatenate(plans) if plans else np.zeros((0, 2)))
        check(self.L.navgpu_tp_update_plans(self.h, first, len(plans), _ptr(xy) if len(xy) else None, _ptr(offsets), int(compute_dists)),
              "tp_update_plans")

    def tp_update_plans_list(self, instances, plans_xy, compute_dists=False):
        """tp_update_plans for a list of robots (strictly increasing indices), plans by list position: one packed upload, one wavefront
        launch, however the robots lie in the fleet."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        plans = [np.ascontiguousarray(p, np.float64).reshape(-1, 2) for p in plans_xy]
        if len(plans) != len(inst):
            raise ValueError("one plan per listed robot")
        offsets = np.zeros(len(plans) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(p) for p in plans])
        xy = np.ascontiguousarray(np.concatenate(plans) if plans else np.zeros((0, 2)))
        check(self.L.navgpu_tp_update_plans_list(self.h, len(inst), _ptr(inst) if len(inst) else None, _ptr(xy) if len(xy) else None,
                                                 _ptr(offsets), int(compute_dists)), "tp_update_plans_list")

    def tp_find_best_path_list(self, instances, pos, vel):
        """tp_find_best_path for a list of robots (strictly increasing indices), pos / vel by list position -> list of TpResult."""
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        vel = np.asarray(vel, np.float32).reshape(-1, 3)
        if len(pos) != len(inst) or len(vel) != len(inst):
            raise ValueError("one pose and one velocity per listed robot")
        n = len(inst)
        st = (N.RobotState * max(n, 1))()
        for k in range(n):
            st[k].pos[:] = [float(v) for v in pos[k]]
            st[k].vel[:] = [float(v) for v in vel[k]]
        out = (N.TpResult * max(n, 1))()
        check(self.L.navgpu_tp_find_best_path_list(self.h, n, _ptr(inst) if n else None, st, out), "tp_find_best_path_list")
        return list(out)[:n]

    @staticmethod
    def _probe_runs(instances, probes, offsets, width):
        inst = np.ascontiguousarray(instances, np.uint32).reshape(-1)
        if offsets is None:
            runs = [np.asarray(p, np.float64).reshape(-1, width) for p in probes]
            off = np.zeros(len(runs) + 1, np.uint32)
            off[1:] = np.cumsum([len(r) for r in runs])
            flat = np.concatenate(runs) if runs else np.zeros((0, width))
        else:
            off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
            flat = np.asarray(probes, np.float64).reshape(-1, width)
        if len(off) != len(inst) + 1 or int(off[-1]) != len(flat):
            raise ValueError("one run of probes per robot (offsets: len(instances) + 1 entries ending at the probe count)")
        return inst, off, np.ascontiguousarray(flat, np.float64)

    def tp_score_trajectories(self, instances, probes, offsets=None):
        """TrajectoryPlanner::scoreTrajectory / checkTrajectory for a list of robots (strictly increasing indices), each with a run of
        probes of 9 doubles (pose x y theta, velocity x y theta, sample x y theta), in one launch.  probes: a list of (n_k, 9) arrays,
        one per robot, or - with offsets - one flat (total, 9) array.  Returns (costs, ok) per probe, in probe order."""
        inst, off, flat = self._probe_runs(instances, probes, offsets, 9)
        costs = np.zeros(max(len(flat), 1), np.float64)
        ok = np.zeros(max(len(flat), 1), np.int32)
        check(self.L.navgpu_tp_score_trajectories(self.h, len(inst), _ptr(inst), _ptr(off), _ptr(flat), _ptr(costs), _ptr(ok)),
              "tp_score_trajectories")
        return costs[:len(flat)].copy(), ok[:len(flat)].astype(bool)

    # ---------------------------------------------------------------- TrajectoryPlannerROS control cycle
    def configure_tp_ros(self, params=None, **kw):
        """TrajectoryPlannerROS's own parameters (navgpu_tp_ros_params); the planner's come from configure_trajectory_planner."""
        p = params if params is not None else N.TpRosParams(**kw)
        check(self.L.navgpu_tp_ros_configure(self.h, C.byref(p)), "tp_ros_configure")

    def tp_ros_set_plans(self, plans_xyyaw, plans_to_global=None, first=0):
        """TrajectoryPlannerROS::setPlan for robots first .. first + len(plans) - 1."""
        plans = [np.ascontiguousarray(p, np.float64).reshape(-1, 3) for p in plans_xyyaw]
        offsets = np.zeros(len(plans) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(p) for p in plans])
        poses = np.ascontiguousarray(np.concatenate(plans) if plans else np.zeros((0, 3)))
        T = None if plans_to_global is None else np.ascontiguousarray(plans_to_global, np.float64).reshape(len(plans), 3)
        check(self.L.navgpu_tp_ros_set_plans(self.h, first, len(plans), _ptr(poses) if len(poses) else None, _ptr(offsets),
                                             None if T is None else _ptr(T)), "tp_ros_set_plans")

    def tp_ros_compute_velocity_commands(self, poses, odom_vels, first=0, have_pose=None):
        """TrajectoryPlannerROS::computeVelocityCommands for len(poses) robots -> list of CmdResult."""
        arr = self._robot_inputs(poses, odom_vels, have_pose)
        out = (N.CmdResult * len(arr))()
        check(self.L.navgpu_tp_ros_compute_velocity_commands(self.h, first, len(arr), arr, out), "tp_ros_compute_velocity_commands")
        return list(out)

    def tp_ros_is_goal_reached(self, first=0, count=None):
        first, count = self._range(first, count)
        out = (C.c_int32 * count)()
        check(self.L.navgpu_tp_ros_is_goal_reached(self.h, first, count, out), "tp_ros_is_goal_reached")
        return [bool(v) for v in out]

    def tp_ros_check_trajectories(self, instances, poses, odom_vels, vel_samples, update_map=False, have_pose=None, offsets=None):
        """TrajectoryPlannerROS::scoreTrajectory / checkTrajectory(vx, vy, vtheta, update_map) for a list of robots: poses / odom_vels /
        have_pose per listed robot, vel_samples a list of (n_k, 3) arrays (or flat with offsets).  Returns (costs, ok) per probe."""
        inst, off, flat = self._probe_runs(instances, vel_samples, offsets, 3)
        arr = self._robot_inputs(poses, odom_vels, have_pose)
        if len(arr) != len(inst):
            raise ValueError("tp_ros_check_trajectories: one pose per listed robot")
        costs = np.zeros(max(len(flat), 1), np.float64)
        ok = np.zeros(max(len(flat), 1), np.int32)
        check(self.L.navgpu_tp_ros_check_trajectories(self.h, len(inst), _ptr(inst), arr, _ptr(off), _ptr(flat), int(bool(update_map)),
                                                      _ptr(costs), _ptr(ok)), "tp_ros_check_trajectories")
        return costs[:len(flat)].copy(), ok[:len(flat)].astype(bool)

    def _tp_ros_plan(self, fn, what, instance):
        n = check(fn(self.h, instance, None, 0), what)
        out = np.zeros((n, 3))
        if n:
            check(fn(self.h, instance, _ptr(out), n), what)
        return out

    def tp_ros_global_plan(self, instance):
        """global_plan_ of the robot after pruning, (n, 3)."""
        return self._tp_ros_plan(self.L.navgpu_tp_ros_get_plan, "tp_ros_get_plan", instance)

    def tp_ros_transformed_plan(self, instance):
        """The transformed (and pruned) window of the robot's last cycle, (m, 3): what g_plan_pub_ publishes."""
        return self._tp_ros_plan(self.L.navgpu_tp_ros_transformed_plan, "tp_ros_transformed_plan", instance)

    # ---------------------------------------------------------------- footprint queries, rotate recovery, carrot planner
    def footprint_cost(self, poses, first=0, allow_unknown=True, want_first_illegal=True):
        """CostmapModel::footprintCost of runs of poses: `poses` is one (q_k, 3) array of x, y, theta per robot from `first` on
        (empty runs allowed).  Returns (list of cost arrays, first illegal index per robot or -1)."""
        runs = [np.asarray(p, np.float64).reshape(-1, 3) for p in poses]
        counts = np.array([len(r) for r in runs], np.uint32)
        packed = np.ascontiguousarray(np.concatenate(runs) if runs else np.zeros((0, 3)))
        costs = np.zeros(len(packed), np.float64)
        fi = np.zeros(len(runs), np.int32)
        check(self.L.navgpu_footprint_cost(self.h, first, len(runs), _ptr(counts), _ptr(packed), int(allow_unknown), _ptr(costs),
                                           _ptr(fi) if want_first_illegal else None), "footprint_cost")
        off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        return [costs[off[k]:off[k + 1]] for k in range(len(runs))], fi

    def configure_rotate_recovery(self, params=None, **kw):
        p = params if params is not None else N.RotateRecoveryParams(**kw)
        check(self.L.navgpu_rotate_recovery_configure(self.h, C.byref(p)), "rotate_recovery_configure")

    def rotate_recovery_step(self, poses, states, first=0):
        """One pass of RotateRecovery::runBehavior's loop for len(poses) robots.  `states` is a ctypes array of
        RotateRecoveryState, updated in place (zero-initialised states begin a run).  Returns (cmd_wz, status)."""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        wz = np.zeros(len(p), np.float64)
        status = np.zeros(len(p), np.int32)
        check(self.L.navgpu_rotate_recovery_step(self.h, first, len(p), _ptr(p), C.cast(states, C.c_void_p), _ptr(wz), _ptr(status)),
              "rotate_recovery_step")
        return wz, status

    def carrot_plan(self, starts, goals, first=0, allow_unknown=True):
        """CarrotPlanner::makePlan's search for len(starts) plans -> (targets (n, 3), found (n,): candidates tried, 0 = none legal)."""
        s = np.ascontiguousarray(starts, np.float64).reshape(-1, 3)
        g = np.ascontiguousarray(goals, np.float64).reshape(-1, 3)
        targets = np.zeros_like(s)
        found = np.zeros(len(s), np.int32)
        check(self.L.navgpu_carrot_plan(self.h, first, len(s), _ptr(s), _ptr(g), int(allow_unknown), _ptr(targets), _ptr(found)), "carrot_plan")
        return targets, found

    # ---------------------------------------------------------------- voxel layer debug outputs
    def voxel_points(self, status, as_double=False, first=0, count=None):
        """The voxels whose VoxelGrid::getVoxel equals `status` (N.VOXEL_UNKNOWN / N.VOXEL_MARKED) as world coordinates of
        their centres, in the reference's loop order (y, x, z): one (k, 3) float32 / float64 array per robot.  Counts first,
        then sizes the buffer from the largest count."""
        first, count = self._range(first, count)
        counts = np.zeros(count, np.uint32)
        check(self.L.navgpu_voxel_points(self.h, first, count, int(status), int(as_double), 0, None, _ptr(counts)), "voxel_points")
        cap = int(counts.max())
        xyz = np.zeros((count, cap, 3), np.float64 if as_double else np.float32)
        if cap:
            check(self.L.navgpu_voxel_points(self.h, first, count, int(status), int(as_double), cap, _ptr(xyz), _ptr(counts)), "voxel_points")
        return [xyz[k, :counts[k]] for k in range(count)]

    def voxel_clearing_endpoints(self, first=0, count=None):
        """The clearing_endpoints clouds of the last staged and updated cycle: per robot a list with one (k, 3) float32 array
        per staged observation, in staging order (empty for marking-only ones)."""
        first, count = self._range(first, count)
        max_obs = max(1, self.desc.max_observations)
        counts = np.zeros(count, np.uint32)
        per_obs = np.zeros((count, max_obs), np.uint32)
        check(self.L.navgpu_voxel_clearing_endpoints(self.h, first, count, 0, None, _ptr(per_obs), _ptr(counts)), "voxel_clearing_endpoints")
        cap = int(counts.max())
        xyz = np.zeros((count, cap, 3), np.float32)
        if cap:
            check(self.L.navgpu_voxel_clearing_endpoints(self.h, first, count, cap, _ptr(xyz), _ptr(per_obs), _ptr(counts)),
                  "voxel_clearing_endpoints")
        off = np.concatenate([np.zeros((count, 1), np.int64), np.cumsum(per_obs, axis=1, dtype=np.int64)], axis=1)
        return [[xyz[k, off[k, o]:off[k, o + 1]] for o in range(max_obs)] for k in range(count)]

    # ---------------------------------------------------------------- measurement
    def profile(self, enable=True):
        check(self.L.navgpu_profile_enable(self.h, int(enable)), "profile_enable")

    def profile_reset(self):
        check(self.L.navgpu_profile_reset(self.h), "profile_reset")

    def profile_select(self, names=None):
        """Bracket only the named kernels with events while profiling (None = all)."""
        mask = 0xFFFFFFFF if names is None else sum(1 << N.KERNELS.index(k) for k in names)
        check(self.L.navgpu_profile_select(self.h, mask), "profile_select")

    def profile_read(self):
        out = {}
        for k, name in enumerate(N.KERNELS):
            ms, n = C.c_double(), C.c_uint64()
            check(self.L.navgpu_profile_read(self.h, k, C.byref(ms), C.byref(n)), "profile_read")
            out[name] = (ms.value, n.value)
        return out
