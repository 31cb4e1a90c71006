// Device side of navgpu_navfn_ros_* (navfn_ros_kernels.hip): NavfnROS round navfn::NavFn, for a batch of plans.
#pragma once
#include "navgpu_device.h"

namespace navgpu {

constexpr int kNrMaxWindow = 4096;  // candidates per axis of a tolerance window (NAVGPU_NAVFN_ROS_MAX_WINDOW)

// One tolerance window (navfn_ros.cpp:301-327, 130-155): the plan (relative to the call's first) whose potential it reads, that
// plan's frame, the pose the window is centred on, the weights, and where its two coordinate sequences (ny values of p.y, then
// nx values of p.x, as the reference's += resolution sums them) begin in the call's sequence buffer.  ny = 0: nothing to scan.
struct NrWindow {
  double origin_x, origin_y, resolution;
  double goal_x, goal_y;
  double w_dist, w_len;
  uint32_t plan, seq, ny, nx;
  int32_t use_alt, pad;
};
// What a window found: how many candidates had a potential below POT_HIGH, and the first one in scan order (y outer, x inner) of
// the lowest cost below DBL_MAX: its scan index (-1: none), coordinates, cell and cost.
struct NrBest {
  double x, y, cost;
  int32_t index, candidates;
  int32_t cell[2];
};
// A second calcPath (getPlanFromPotential, navfn_ros.cpp:426-437) of plan first + k: from `start` (-1: none; with from_best,
// taken from best[k] instead) to `goal` over the array the plan's result is in.  The kernel fills `first_pass` with the plan's
// result record as it was before the walk and `length` with the walk's.
struct NrPathJob {
  int32_t start[2], goal[2];
  int32_t from_best, use_alt, length, pad;
  navgpu_navfn_result first_pass;
};
// The potential cloud's view of plan first + k: frame, NavFn's start cell (whose potential divides) and the array to read
struct NrCloudPlan {
  double origin_x, origin_y, resolution;
  int32_t start_cell, use_alt;
};
struct NrCloudPoint {  // PotarrPoint (navfn/potarr_point.h)
  float x, y, z, pot_value;
};

constexpr uint32_t kNrChunk = 1024;  // cells of a cloud chunk: 256 lanes x 4
inline uint32_t nrCloudChunks(int ns) { return ((uint32_t)ns + kNrChunk - 1) / kNrChunk; }

// best[j] of windows[j], j < n_windows; any_only: only `candidates` (0 / 1, an OR) is filled
void launch_nr_window(const NavfnDev& nv, uint32_t first, const NrWindow* windows, const double* seq, uint32_t n_windows, int any_only, NrBest* best,
                      hipStream_t s);
// the second calcPath of jobs[k], k < count, into plan first + k's path buffer and result record; n_max = 4 * nx
void launch_nr_path(const NavfnDev& nv, uint32_t first, uint32_t count, NrPathJob* jobs, const NrBest* best, hipStream_t s);
// xy_out[2 q] = (double)potential at the cell of point q of plan first + qplan[q], DBL_MAX off the map (xy_out[2 q + 1] untouched)
void launch_nr_point_potential(const NavfnDev& nv, uint32_t first, const NrCloudPlan* plans, const int32_t* qplan, double* xy, uint32_t n_queries,
                               hipStream_t s);
// totals[k * chunks + c] = exclusive prefix over all (plan, chunk) pairs of the cells with potential < 10e7; offsets[0 .. count]
void launch_nr_cloud_count(const NavfnDev& nv, uint32_t first, uint32_t count, const NrCloudPlan* plans, uint32_t* totals, uint32_t* offsets,
                           hipStream_t s);
void launch_nr_cloud_emit(const NavfnDev& nv, uint32_t first, uint32_t count, const NrCloudPlan* plans, const uint32_t* totals, NrCloudPoint* points,
                          uint32_t capacity, hipStream_t s);

}  // namespace navgpu
