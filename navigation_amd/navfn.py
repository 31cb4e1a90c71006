"""NavFn: thin Python handle over navgpu_navfn_* — navfn::NavFn (navfn/src/navfn.cpp) for a batch of plans on one GPU.

  set_costmap   NavFn::setCostmap                        (navfn.cpp:222-283)
  plan          NavFn::setGoal / setStart + calcNavFnDijkstra | calcNavFnAstar   (navfn.cpp:145-171, 293-345)
  path          NavFn::getPathX / getPathY / getPathLen
  potential     NavFn::potarr
  costarr       NavFn::costarr
  make_plan     GlobalPlanner::makePlan                  (global_planner/src/planner_core.cpp:222-327)
  plans         the plans makePlan fills, concatenated   (planner_core.cpp:306-321, 351-395; orientation_filter.cpp:53-111)
  potential_grid  GlobalPlanner::publishPotential's data (planner_core.cpp:417-434)
  navfn_ros_make_plan / navfn_ros_plans   NavfnROS::makePlan                 (navfn/src/navfn_ros.cpp:218-374)
  navfn_ros_plan_from_potential           NavfnROS::getPlanFromPotential     (:400-461)
  navfn_ros_compute_potential             NavfnROS::computePotential         (:171-197)
  navfn_ros_point_potential / navfn_ros_valid_point_potential   getPointPotential / validPointPotential (:130-169)
  navfn_ros_potential_cloud               the `potential` topic's cloud      (:342-368)
  plan_service / plan_service_candidates  MoveBase::planService's goal search (move_base/src/move_base.cpp:365-417)
All compute happens in libnavgpu.so on the GPU; this file only marshals numpy buffers.
"""
import ctypes as C

import numpy as np

from ._lib import (PLAN_FAMILY_GLOBAL_PLANNER, GlobalPlannerParams, GlobalPose, MakePlanOptions, MakePlanResult, NavfnResult,
                   NavfnRosCloudPoint, NavfnRosParams, NavfnRosResult, PlanServiceRequest, PlanServiceResult, check, lib)


class NavFn:
    def __init__(self, nx, ny, n_plans=1, device=0):
        self.L = lib()
        self.nx, self.ny, self.n = nx, ny, n_plans
        h = C.c_void_p()
        check(self.L.navgpu_navfn_create(nx, ny, n_plans, device, C.byref(h)), "navgpu_navfn_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.navgpu_navfn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_costmap(self, cmap, first=0, count=None, cost_mode=1, allow_unknown=True):
        """cmap: (ny, nx) shared by `count` plans, or (count, ny, nx).  cost_mode 1: costmap_2d values (isROS), 2: plain PGM,
        0: the bytes are costarr itself."""
        a = np.ascontiguousarray(cmap, np.uint8)
        shared = a.ndim == 2
        count = (self.n - first) if count is None else count
        if not shared:
            assert a.shape[0] == count
        assert a.shape[-2:] == (self.ny, self.nx)
        check(self.L.navgpu_navfn_set_costmap(self.h, first, count, a.ctypes.data_as(C.c_void_p), int(shared), cost_mode, int(allow_unknown)),
              "navfn_set_costmap")

    def set_costmap_from_fleet(self, fleet, first=0, count=None, fleet_first=0, allow_unknown=True):
        count = (self.n - first) if count is None else count
        check(self.L.navgpu_navfn_set_costmap_from_fleet(self.h, first, count, fleet.h, fleet_first, int(allow_unknown)), "navfn_set_costmap_from_fleet")

    def set_costmap_from_fleet_instance(self, fleet, instance, first=0, count=None, cost_mode=1, allow_unknown=True):
        """every plan of the range takes the master grid of ONE fleet instance (the slots of a plan_service request)"""
        count = (self.n - first) if count is None else count
        check(self.L.navgpu_navfn_set_costmap_from_fleet_instance(self.h, first, count, fleet.h, instance, cost_mode, int(allow_unknown)),
              "navfn_set_costmap_from_fleet_instance")

    def plan(self, goals, starts, first=0, astar=False, at_start=True):
        g = np.ascontiguousarray(goals, np.int32).reshape(-1, 2)
        s = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
        assert len(g) == len(s)
        res = (NavfnResult * len(g))()
        check(self.L.navgpu_navfn_plan(self.h, first, len(g), g.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), int(astar), int(at_start),
                                       C.cast(res, C.c_void_p)), "navfn_plan")
        return list(res)

    def plan_wavefront(self, goals, starts, first=0, at_start=True):
        """navgpu_navfn_plan_wavefront: the expansion as a tiled wavefront (the update rule's fixed point; Dijkstra only)."""
        g = np.ascontiguousarray(goals, np.int32).reshape(-1, 2)
        s = np.ascontiguousarray(starts, np.int32).reshape(-1, 2)
        assert len(g) == len(s)
        res = (NavfnResult * len(g))()
        check(self.L.navgpu_navfn_plan_wavefront(self.h, first, len(g), g.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), int(at_start),
                                                 C.cast(res, C.c_void_p)), "navfn_plan_wavefront")
        return list(res)

    def global_planner_plan(self, starts_xy, goals_xy, goal_cells, first=0, wavefront=False, **params):
        """GlobalPlanner::makePlan's expansion + traceback (map coordinates; costs set with cost_mode=0).  wavefront: the
        Dijkstra expansion as the tiled wavefront (navgpu_global_planner_plan_wavefront)."""
        st = np.ascontiguousarray(starts_xy, np.float64).reshape(-1, 2)
        gl = np.ascontiguousarray(goals_xy, np.float64).reshape(-1, 2)
        gc = np.ascontiguousarray(goal_cells, np.int32).reshape(-1, 2)
        gp = GlobalPlannerParams(**params)
        res = (NavfnResult * len(st))()
        fn = self.L.navgpu_global_planner_plan_wavefront if wavefront else self.L.navgpu_global_planner_plan
        check(fn(self.h, first, len(st), C.byref(gp), st.ctypes.data_as(C.c_void_p), gl.ctypes.data_as(C.c_void_p),
                 gc.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)), "global_planner_plan")
        return list(res)

    def make_plan(self, frames, starts_xyyaw, goals_xyyaw, first=0, orientation_mode=0, wavefront=False, **params):
        """navgpu_global_planner_make_plan: GlobalPlanner::makePlan from world poses (costs set with cost_mode=0).  frames:
        (count, 3) {origin_x, origin_y, resolution}, or one triple for every plan.  Returns a list of MakePlanResult; a plan
        whose status is not MAKE_PLAN_OK has no poses and does not fail the call."""
        st = np.ascontiguousarray(starts_xyyaw, np.float64).reshape(-1, 3)
        gl = np.ascontiguousarray(goals_xyyaw, np.float64).reshape(-1, 3)
        assert len(st) == len(gl)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(frames, np.float64).reshape(-1, 3), (len(st), 3)))
        gp = GlobalPlannerParams(**params)
        opt = MakePlanOptions(int(orientation_mode), int(wavefront))
        res = (MakePlanResult * len(st))()
        check(self.L.navgpu_global_planner_make_plan(self.h, first, len(st), C.byref(gp), C.byref(opt), fr.ctypes.data_as(C.c_void_p),
                                                     st.ctypes.data_as(C.c_void_p), gl.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)),
              "global_planner_make_plan")
        return list(res)

    def plans(self, first=0, count=None, capacity=None):
        """navgpu_global_planner_plans: (poses (total, 3) float64 {x, y, yaw}, offsets (count + 1,) uint32) of the last make_plan
        over the range; plan first + k is poses[offsets[k]:offsets[k + 1]].  capacity: write at most that many poses (the
        offsets stay true); 0 counts only."""
        count = (self.n - first) if count is None else count
        offsets = np.zeros(count + 1, np.uint32)
        if capacity is None:
            check(self.L.navgpu_global_planner_plans(self.h, first, count, 0, None, offsets.ctypes.data_as(C.c_void_p)), "global_planner_plans")
            capacity = int(offsets[-1])
        poses = np.zeros((capacity, C.sizeof(GlobalPose) // 8), np.float64)
        if capacity:
            check(self.L.navgpu_global_planner_plans(self.h, first, count, capacity, poses.ctypes.data_as(C.c_void_p),
                                                     offsets.ctypes.data_as(C.c_void_p)), "global_planner_plans")
        return poses, offsets

    def potential_grid(self, first=0, count=None, publish_scale=100):
        """navgpu_global_planner_potential_grid: (grids (count, ny, nx) int8, maxima (count,) float32)."""
        count = (self.n - first) if count is None else count
        grids = np.zeros((count, self.ny, self.nx), np.int8)
        maxima = np.zeros(count, np.float32)
        check(self.L.navgpu_global_planner_potential_grid(self.h, first, count, int(publish_scale), grids.ctypes.data_as(C.c_void_p),
                                                          maxima.ctypes.data_as(C.c_void_p)), "global_planner_potential_grid")
        return grids, maxima

    def _frames(self, frames, count):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(frames, np.float64).reshape(-1, 3), (count, 3)))

    def navfn_ros_make_plan(self, frames, starts_xyyaw, goals_xyyaw, tolerances=0.0, first=0, w_dist=1.0, w_len=0.0, wavefront=False):
        """navgpu_navfn_ros_make_plan: NavfnROS::makePlan from world poses (costs set with cost_mode=1 or from a fleet).
        tolerances: one per plan, or one for all.  Returns a list of NavfnRosResult."""
        st = np.ascontiguousarray(starts_xyyaw, np.float64).reshape(-1, 3)
        gl = np.ascontiguousarray(goals_xyyaw, np.float64).reshape(-1, 3)
        assert len(st) == len(gl)
        fr = self._frames(frames, len(st))
        tol = np.ascontiguousarray(np.broadcast_to(np.asarray(tolerances, np.float64).reshape(-1), (len(st),)))
        pr = NavfnRosParams(float(w_dist), float(w_len), int(wavefront), 0)
        res = (NavfnRosResult * len(st))()
        check(self.L.navgpu_navfn_ros_make_plan(self.h, first, len(st), C.byref(pr), fr.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p),
                                                gl.ctypes.data_as(C.c_void_p), tol.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)),
              "navfn_ros_make_plan")
        return list(res)

    def navfn_ros_plans(self, first=0, count=None, capacity=None):
        """navgpu_navfn_ros_plans: (poses (total, 3) float64 {x, y, yaw}, offsets (count + 1,) uint32), as plans()."""
        count = (self.n - first) if count is None else count
        offsets = np.zeros(count + 1, np.uint32)
        if capacity is None:
            check(self.L.navgpu_navfn_ros_plans(self.h, first, count, 0, None, offsets.ctypes.data_as(C.c_void_p)), "navfn_ros_plans")
            capacity = int(offsets[-1])
        poses = np.zeros((capacity, C.sizeof(GlobalPose) // 8), np.float64)
        check(self.L.navgpu_navfn_ros_plans(self.h, first, count, capacity, poses.ctypes.data_as(C.c_void_p) if capacity else None,
                                            offsets.ctypes.data_as(C.c_void_p)), "navfn_ros_plans")
        return poses[:min(capacity, int(offsets[-1]))], offsets

    def navfn_ros_plan_from_potential(self, frames, goals_xyyaw, first=0):
        """navgpu_navfn_ros_plan_from_potential: getPlanFromPotential on the potential each plan holds; navfn_ros_plans reads the plans."""
        gl = np.ascontiguousarray(goals_xyyaw, np.float64).reshape(-1, 3)
        fr = self._frames(frames, len(gl))
        res = (NavfnRosResult * len(gl))()
        check(self.L.navgpu_navfn_ros_plan_from_potential(self.h, first, len(gl), fr.ctypes.data_as(C.c_void_p), gl.ctypes.data_as(C.c_void_p),
                                                          C.cast(res, C.c_void_p)), "navfn_ros_plan_from_potential")
        return list(res)

    def navfn_ros_compute_potential(self, frames, points_xy, first=0, wavefront=False):
        """navgpu_navfn_ros_compute_potential: computePotential of one world point per plan."""
        pt = np.ascontiguousarray(points_xy, np.float64).reshape(-1, 2)
        fr = self._frames(frames, len(pt))
        pr = NavfnRosParams(1.0, 0.0, int(wavefront), 0)
        res = (NavfnRosResult * len(pt))()
        check(self.L.navgpu_navfn_ros_compute_potential(self.h, first, len(pt), C.byref(pr), fr.ctypes.data_as(C.c_void_p),
                                                        pt.ctypes.data_as(C.c_void_p), C.cast(res, C.c_void_p)), "navfn_ros_compute_potential")
        return list(res)

    def _queries(self, frames, points_xy, first, count):
        """points_xy: one (m_k, 2) array per plan -> (frames, counts, packed points)"""
        count = (self.n - first) if count is None else count
        per_plan = [np.asarray(p, np.float64).reshape(-1, 2) for p in points_xy]
        assert len(per_plan) == count
        counts = np.array([len(p) for p in per_plan], np.uint32)
        packed = np.ascontiguousarray(np.concatenate(per_plan) if per_plan else np.zeros((0, 2)))
        return count, self._frames(frames, count), counts, packed

    def navfn_ros_point_potential(self, frames, points_xy, first=0, count=None):
        """navgpu_navfn_ros_point_potential: points_xy is one (m_k, 2) array per plan; returns the packed float64 potentials."""
        count, fr, counts, packed = self._queries(frames, points_xy, first, count)
        out = np.zeros(len(packed), np.float64)
        check(self.L.navgpu_navfn_ros_point_potential(self.h, first, count, fr.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                      packed.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), "navfn_ros_point_potential")
        return out

    def navfn_ros_valid_point_potential(self, frames, points_xy, tolerances, first=0, count=None):
        """navgpu_navfn_ros_valid_point_potential: tolerances packed like the points (or one for all); returns int32 flags."""
        count, fr, counts, packed = self._queries(frames, points_xy, first, count)
        tol = np.ascontiguousarray(np.broadcast_to(np.asarray(tolerances, np.float64).reshape(-1), (len(packed),)))
        out = np.zeros(len(packed), np.int32)
        check(self.L.navgpu_navfn_ros_valid_point_potential(self.h, first, count, fr.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                            packed.ctypes.data_as(C.c_void_p), tol.ctypes.data_as(C.c_void_p),
                                                            out.ctypes.data_as(C.c_void_p)), "navfn_ros_valid_point_potential")
        return out

    def navfn_ros_potential_cloud(self, frames, first=0, count=None, capacity=None):
        """navgpu_navfn_ros_potential_cloud: (points (total, 4) float32 {x, y, z, pot_value}, offsets (count + 1,) uint32)."""
        count = (self.n - first) if count is None else count
        fr = self._frames(frames, count)
        offsets = np.zeros(count + 1, np.uint32)
        if capacity is None:
            check(self.L.navgpu_navfn_ros_potential_cloud(self.h, first, count, fr.ctypes.data_as(C.c_void_p), 0, None,
                                                          offsets.ctypes.data_as(C.c_void_p)), "navfn_ros_potential_cloud")
            capacity = int(offsets[-1])
        pts = np.zeros((capacity, C.sizeof(NavfnRosCloudPoint) // 4), np.float32)
        check(self.L.navgpu_navfn_ros_potential_cloud(self.h, first, count, fr.ctypes.data_as(C.c_void_p), capacity,
                                                      pts.ctypes.data_as(C.c_void_p) if capacity else None, offsets.ctypes.data_as(C.c_void_p)),
              "navfn_ros_potential_cloud")
        return pts[:min(capacity, int(offsets[-1]))], offsets

    def plan_service_candidates(self, goal_xy, resolution, tolerance):
        """planService's candidate goals, the exact goal first: (n, 2) float64"""
        g = np.ascontiguousarray(goal_xy, np.float64).reshape(2)
        n = check(self.L.navgpu_move_base_plan_service_candidates(g.ctypes.data_as(C.c_void_p), float(resolution), float(tolerance), 0, None),
                  "move_base_plan_service_candidates")
        out = np.zeros((n, 2))
        check(self.L.navgpu_move_base_plan_service_candidates(g.ctypes.data_as(C.c_void_p), float(resolution), float(tolerance), n,
                                                              out.ctypes.data_as(C.c_void_p)), "move_base_plan_service_candidates")
        return out

    def plan_service(self, family, requests, slots_per_request, first_slot=0, orientation_mode=0, wavefront=False, w_dist=1.0, w_len=0.0,
                     **params):
        """navgpu_move_base_plan_service: MoveBase::planService's goal search for a list of requests - dicts with start, goal
        (x, y, yaw), frame (origin_x, origin_y, resolution), tolerance and, for the navfn_ros family, default_tolerance.  Request q
        owns the slots first_slot + q * slots_per_request ...; their costs must be set.  Returns (list of PlanServiceResult, list of
        the winners' make_plan results); the winner's plan is read with plans() / navfn_ros_plans(first=result.slot, count=1)."""
        arr = (PlanServiceRequest * len(requests))()
        for a, r in zip(arr, requests):
            a.start[:] = [float(v) for v in r["start"]]
            a.goal[:] = [float(v) for v in r["goal"]]
            a.frame[:] = [float(v) for v in r["frame"]]
            a.tolerance = float(r["tolerance"])
            a.default_tolerance = float(r.get("default_tolerance", 0.0))
        res = (PlanServiceResult * len(requests))()
        is_gp = int(family) == PLAN_FAMILY_GLOBAL_PLANNER
        won = ((MakePlanResult if is_gp else NavfnRosResult) * len(requests))()
        gp, opt = GlobalPlannerParams(**params), MakePlanOptions(int(orientation_mode), int(wavefront))
        nr = NavfnRosParams(float(w_dist), float(w_len), int(wavefront), 0)
        check(self.L.navgpu_move_base_plan_service(self.h, first_slot, int(slots_per_request), len(requests), int(family),
                                                   C.byref(gp) if is_gp else None, C.byref(opt) if is_gp else None, None if is_gp else C.byref(nr),
                                                   C.cast(arr, C.c_void_p), C.cast(res, C.c_void_p), C.cast(won, C.c_void_p)),
              "move_base_plan_service")
        return list(res), list(won)

    def path(self, plan=0):
        n = check(self.L.navgpu_navfn_path(self.h, plan, None, 0), "navfn_path")
        out = np.zeros((max(n, 1), 2), np.float32)
        if n:
            check(self.L.navgpu_navfn_path(self.h, plan, out.ctypes.data_as(C.c_void_p), n), "navfn_path")
        return out[:n].copy()

    def potential(self, plan=0):
        out = np.zeros((self.ny, self.nx), np.float32)
        check(self.L.navgpu_navfn_potential(self.h, plan, out.ctypes.data_as(C.c_void_p)), "navfn_potential")
        return out

    def costarr(self, plan=0):
        """NavFn::costarr as the last set_costmap / set_costmap_from_fleet left it, (ny, nx) uint8."""
        out = np.zeros((self.ny, self.nx), np.uint8)
        check(self.L.navgpu_navfn_costarr(self.h, plan, out.ctypes.data_as(C.c_void_p)), "navfn_costarr")
        return out
