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

// ---- the layered map update (costmap3d_layer_kernels.hip, include/navgpu_costmap3d_layers.h) ----
// A tile is 64 consecutive column words of a row (a wave's lanes): tpr tiles per row, tiles = tpr * sy per instance, one bit each
// in bitmaps of tw 32-bit words.  nc costmap layers (POINT_CLOUD, STATIC_2D) have a slot each.
struct C3dLayersDev {
  uint64_t* sets = nullptr;     // [n][nc][2][3][cols] a layer's two plane sets (LETHAL, NONLETHAL, FREE): the current one and the next scratch
  uint64_t* changed = nullptr;  // [n][nc][cols] CostmapLayer3D::changed_cells_
  uint32_t* occ = nullptr;      // [n][nc][2][tw] tiles a plane set occupies
  uint32_t* dirty = nullptr;    // [n][tw] tiles with a changed bit in some layer
  uint64_t* free_plane = nullptr;  // [n][cols] the master's FREE plane
  uint8_t* layer2d = nullptr;   // [n][cols] Costmap3DTo2DLayer's costmap_
  uint32_t nc = 0, tpr = 0, tiles = 0, tw = 0;
  int32_t nonlethal_cost_2d = 127;
  int32_t all_tiles = 0;        // tool builds: the plain full-volume pass, no tile is skipped
  double inv_res = 0;           // 1.0 / resolution (octomap's resolution_factor)
  __host__ __device__ uint64_t* set(uint32_t inst, uint32_t slot, uint32_t which, uint32_t cols) const {
    return sets + (((size_t)inst * nc + slot) * 2 + which) * 3 * cols;
  }
  __host__ __device__ uint32_t* occOf(uint32_t inst, uint32_t slot, uint32_t which) const { return occ + (((size_t)inst * nc + slot) * 2 + which) * tw; }
};
enum { kC3dL = 0, kC3dN = 1, kC3dF = 2 };  // plane order inside a set

// one (instance, layer) pair of a buffer_clouds / set_static_grid call
struct C3dCloudRec {
  double tf[12];
  int64_t ok[3];        // llround(origin / resolution)
  uint32_t instance, slot, next;  // next: the set that receives the new cells (the other one is current)
  uint32_t first_point, n_points, has_intensity;
  float free_intensity, lethal_intensity;
};
struct C3dGridRec {
  int64_t ok[3];
  double origin_x, origin_y, height;
  uint32_t instance, slot, next, width, rows;
  int32_t threshold, unknown_to_lethal;
};
// one cylinder layer of one listed instance of an update
struct C3dCylRec {
  double cx, cy, px, py, r;  // current and previous robot position, the radius
  int32_t cbox[4], pbox[4];  // clamped key boxes x0, x1, y0, y1 (inclusive)
  int32_t has_cur, has_prev;
};
struct C3dLayerRule {  // one layer of the stack, in order
  int32_t kind, enabled, method, index;  // index: the slot of a costmap layer, the number of a cylinder layer
};
struct C3dUpdate {
  const uint32_t* instances;  // [n]
  const uint32_t* cur;        // [n][nc] the current set of each slot
  const uint32_t* full;       // [n]
  const int64_t* ok;          // [n][3]
  const C3dCylRec* cyl;       // [n][n_cyl]
  int32_t* box;               // [n][4] x0, y0, x1, y1 of the columns with a bounds bit: min, min, max, max
  uint32_t n, n_cyl, n_layers;
  C3dLayerRule rules[8];
};
struct C3dCosts2d {
  const uint32_t* instances;
  const int32_t* boxes;  // [n][4] min_i, min_j, max_i, max_j
  uint8_t* grid;
  size_t stride;
  uint32_t n;
  int32_t use_maximum;
};

void launch_c3d_cloud(const C3dDev& d, const C3dLayersDev& ly, const C3dCloudRec* clouds, uint32_t n_clouds, uint32_t max_points, const float* points,
                      uint32_t* clipped, hipStream_t stream);
void launch_c3d_static2d(const C3dDev& d, const C3dLayersDev& ly, const C3dGridRec* rec, size_t cells, const int8_t* grid, uint32_t* clipped,
                         hipStream_t stream);
// mode 0: the swap of every listed pair; mode 1: touch (changed |= present) of the pairs' current sets (next names the other one)
void launch_c3d_layer_swap(const C3dDev& d, const C3dLayersDev& ly, const uint32_t* pairs3, uint32_t n_pairs, int32_t mode, hipStream_t stream);
void launch_c3d_combine(const C3dDev& d, const C3dLayersDev& ly, const C3dUpdate& u, hipStream_t stream);
void launch_c3d_costs2d(const C3dDev& d, const C3dLayersDev& ly, const C3dCosts2d& c, hipStream_t stream);
void launch_c3d_fill_u8(uint8_t* p, uint8_t v, size_t n, hipStream_t stream);

// ---- rolling maps and resetBoundingBox (costmap3d_roll_kernels.hip, include/navgpu_costmap3d_rolling.h) ----
constexpr uint32_t kC3dRollRow = 2048;  // columns of a row that k_c3d_roll_x holds in registers at a time (256 lanes x 8)
// one moved instance of a roll: dst(x, y) = src(x + dx, y + dy), or empty off the window
struct C3dRollRec {
  double ox, oy;      // the new origin
  uint32_t instance;
  int32_t dx, dy;     // cells; both inside (-size, size) unless empty
  uint32_t cur_bits;  // bit s: the current plane set of slot s; bit 31: |dx| >= size_x or |dy| >= size_y, everything leaves
};
constexpr uint32_t kC3dRollEmpty = 1u << 31;
// one listed instance of a reset_bounding_box call whose clipped box is not empty
struct C3dResetRec {
  uint64_t zmask;
  uint32_t instance, cur_bits;
  uint32_t x0, x1, y0, y1;  // inclusive
};
struct C3dResetSlots {
  uint32_t n, slot[8];  // the POINT_CLOUD slots the mask names
};
// layered: 0 shifts the master's LETHAL and NONLETHAL planes only (ly is not read)
void launch_c3d_roll(const C3dDev& d, const C3dLayersDev& ly, int32_t layered, const C3dRollRec* recs, uint32_t n, bool any_y, bool any_x,
                     hipStream_t stream);
void launch_c3d_reset_box(const C3dDev& d, const C3dLayersDev& ly, const C3dResetRec* recs, uint32_t n, uint32_t max_tiles, const C3dResetSlots& slots,
                          hipStream_t stream);

// ---- publishing: pruned octree leaves out of a handle and into a layer (costmap3d_publish_kernels.hip, include/navgpu_costmap3d_publish.h) ----
// An export works by 64 x 64-column blocks aligned to the lattice, so that a block holds whole octree nodes up to level 6.
struct C3dExportRec {     // one listed instance
  int32_t ok[3];          // the window's lattice origin
  int32_t sd[3];          // shadow column = window column + (sd[0], sd[1]); shadow level = window level + sd[2]
  int32_t bx0, by0;       // the first block: floor(ok / 64)
  uint32_t nbx, nby;      // blocks the window meets
  uint32_t instance, first_block;  // first_block: the instance's first entry in counts / offsets
};
struct C3dExport {
  const C3dExportRec* recs;  // [n]
  const uint64_t* shadow;    // [n_instances][np][cols] the master as last published (DELTA)
  uint32_t* counts;          // [blocks][2] leaves of a block: values, bounds
  uint32_t* offsets;         // [blocks][2] their exclusive prefix over the whole list
  uint32_t* totals;          // [n][4] first_value, n_values, first_bound, n_bounds
  navgpu_c3d_leaf *values, *bounds;
  uint32_t value_capacity, bounds_capacity;
  uint32_t n, blocks, max_blocks;  // max_blocks: the most blocks one listed instance has
  uint32_t np;               // planes of the master: 3 layered, 2 not
  int32_t delta;
};
// one applied message of a layer_update_cells call
struct C3dCellsMsg {
  uint64_t fz[2];        // the forgotten boxes' levels
  int32_t fbox[2][4];    // their columns x0, x1, y0, y1 (inclusive), clipped to the window
  uint32_t instance, slot, cur;
  uint32_t flags;        // bit 0: universe; bits 1..2: the number of forgotten boxes that meet the window
};
struct C3dCells {
  const C3dCellsMsg* msgs;    // [n_msgs]
  const C3dBoxCells* leaves;  // [n_leaves]: cls is the scratch plane (0 E, 1 + class), reserved the message
  uint64_t* scratch;          // [n_msgs][4][cols] E and the value leaves' cells by class; all zero between calls
  uint32_t* touched;          // [n_msgs][tw] tiles with a scratch bit; all zero between calls
  uint32_t n_msgs, n_leaves, max_columns;
};
void launch_c3d_export_count(const C3dDev& d, const C3dLayersDev& ly, const C3dExport& e, hipStream_t stream);  // count, scan, totals
void launch_c3d_export_emit(const C3dDev& d, const C3dLayersDev& ly, const C3dExport& e, hipStream_t stream);
void launch_c3d_shadow_copy(const C3dDev& d, const C3dLayersDev& ly, const C3dExport& e, uint64_t* shadow, hipStream_t stream);
void launch_c3d_cells(const C3dDev& d, const C3dLayersDev& ly, const C3dCells& c, hipStream_t stream);

void launch_c3d_rasterize(const C3dDev& d, uint32_t instance, int32_t mode, const C3dBoxCells* boxes, uint32_t n_boxes,
                          uint32_t max_columns, hipStream_t stream);
void launch_c3d_query(const C3dDev& d, const C3dQuery& q, hipStream_t stream);

}  // namespace navgpu
