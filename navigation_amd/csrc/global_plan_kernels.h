// Device side of navgpu_global_planner_make_plan / _plans / _potential_grid (global_plan_kernels.hip).
#pragma once
#include "navgpu_device.h"

namespace navgpu {

// What k_gp_plan_emit assembles one plan from (getPlanFromPotential's inputs, planner_core.cpp:351-395): the costmap's frame,
// convert_offset, the start's yaw, the goal pose and how many traceback points / poses there are (n_poses 0: no plan).  has_tail: one
// more pose, counted in n_poses, is appended as it is behind the finished plan (planService's push_back(req.goal), move_base.cpp:402).
struct GpPlanRec {
  double origin_x, origin_y, resolution, convert_offset;
  double start_yaw;
  double goal_x, goal_y, goal_yaw;
  int32_t n_path, n_poses, mode, has_tail;
  double tail_x, tail_y, tail_yaw;
};

// Costmap2D::worldToMap (costmap_2d.cpp:208-220) on a map of nx x ny cells.  (int) of a quotient outside int's range is 0x80000000
// on the reference's amd64 builds, which as unsigned fails the size test: restated as "off the map" (a NaN takes the same way).
__host__ __device__ inline bool costmapWorldToMap(double wx, double wy, double origin_x, double origin_y, double resolution, int nx, int ny,
                                                  int32_t cell[2]) {
  if (wx < origin_x || wy < origin_y) return false;
  const double qx = (wx - origin_x) / resolution, qy = (wy - origin_y) / resolution;
  if (!(qx < 2147483648.0) || !(qy < 2147483648.0)) return false;
  cell[0] = (int)qx;
  cell[1] = (int)qy;
  return cell[0] < nx && cell[1] < ny;
}

// costarr[first + k][cells[k]] = FREE_SPACE for cells[k] >= 0
void launch_gp_clear_cells(const NavfnDev& nv, uint32_t first, uint32_t count, const int32_t* cells, hipStream_t s);
// offsets[0 .. count] = exclusive prefix sums of recs[k].n_poses
void launch_gp_plan_scan(const GpPlanRec* recs, uint32_t count, uint32_t* offsets, hipStream_t s);
// poses[offsets[k] + i] = pose i of plan first + k, for offsets[k] + i < capacity (compared in 64 bits: an offset of 0xFFFFFFFF, kPpNoWrite,
// writes nothing whatever the capacity - navgpu_move_base_handover_plans predicates the kernel per plan with it)
void launch_gp_plan_emit(const NavfnDev& nv, uint32_t first, uint32_t count, const GpPlanRec* recs, const uint32_t* offsets, navgpu_global_pose* poses,
                         uint32_t capacity, hipStream_t s);
// grids[k][ns] / maxima[k] from potarr, or potalt where use_alt[k]
void launch_gp_potential_grid(const NavfnDev& nv, uint32_t first, uint32_t count, const uint8_t* use_alt, int32_t publish_scale, int8_t* grids,
                              float* maxima, hipStream_t s);

}  // namespace navgpu
