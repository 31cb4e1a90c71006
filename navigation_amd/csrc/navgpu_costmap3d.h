// The navgpu_costmap3d handle's device view, shared by costmap3d_kernels.hip and navgpu_costmap3d.cpp (include/navgpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/navgpu.h"

namespace navgpu {

constexpr uint32_t kC3dQueue = 4096;      // cells a wave's LDS queue holds: worked off above half, a chunk of columns adds at most half
constexpr uint32_t kC3dMaxColumns = 1u << 26;  // a queue entry is (column << 6) | z

struct C3dDev {
  uint64_t* planes = nullptr;   // [n][2][cols]: LETHAL, NONLETHAL; word index y * sx + x, bit z
  double* origins = nullptr;    // [n][3]
  double* verts = nullptr;      // [max_triangles][3][3] the padded mesh, triangle after triangle, in the robot's frame
  uint32_t n = 0, sx = 0, sy = 0, sz = 0, cols = 0;
  uint32_t nt = 0;
  int32_t closed = 0;
  double res = 0;
};

// one box as the host clipped it to the extents: its columns [x0, x0 + nx) x [y0, y0 + ny), its levels as a mask, its class
struct C3dBoxCells {
  uint64_t zmask;
  uint32_t x0, y0, nx, ny;
  int32_t cls, reserved;
};

// a query call's device buffers: what the one upload carries, and what the one read-back fetches
struct C3dQuery {
  const double* poses;         // [n_poses][7]
  const int32_t* pose_inst;    // [n_poses] the instance of the run that holds the pose, -1: in no run
  const navgpu_c3d_run* runs;  // [n_runs]
  const uint8_t* regions;      // [n_poses]
  const uint8_t* obstacles;    // [n_poses]
  double* pose_costs;          // [n_poses]
  navgpu_c3d_run_result* results;  // [n_runs]
  uint32_t n_poses, n_runs;
  int32_t mode, lazy;
  double scale_y, scale_z, limit;
};

void launch_c3d_rasterize(const C3dDev& d, uint32_t instance, int32_t mode, const C3dBoxCells* boxes, uint32_t n_boxes,
                          uint32_t max_columns, hipStream_t stream);
void launch_c3d_query(const C3dDev& d, const C3dQuery& q, hipStream_t stream);

}  // namespace navgpu
