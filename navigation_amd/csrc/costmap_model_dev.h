// base_local_planner::CostmapModel (costmap_model.cpp:50-142) on a device-resident master grid: pointCost, the LineIterator
// walk behind lineCost and the one-lane footprintCost.  Shared by k_tp_rollout (tp_kernels.hip), which gives a lane a whole
// footprint per rollout step, and k_footprint_cost (footprint_kernels.hip), which gives a lane one edge.
// Compiled with -ffp-contract=off.
#pragma once
#include "navgpu_device.h"

namespace navgpu {

struct CostmapModelDev {
  const uint8_t* master;
  Geom g;
  bool allow_unknown;
  // CostmapModel::pointCost (costmap_model.cpp:133-142) as a predicate on the cell's byte
  __device__ bool pointFails(uint8_t cost) const { return cost == kLethal || (cost == kNoInfo && !allow_unknown); }
  __device__ double pointCost(int x, int y) const {
    const uint8_t cost = master[(uint32_t)y * g.nx + (uint32_t)x];
    if (pointFails(cost)) return -1;
    return cost;
  }
  // The cells of base_local_planner::LineIterator (line_iterator.h:38-139) from (x0, y0) to (x1, y1), both ends included:
  // the longer axis advances with every cell, the shorter one whenever the running remainder - which starts at half the
  // long extent - passes it.  visit(x, y) returns false to end the walk; the return value says whether it ran to the end.
  template <class Visit>
  __device__ static bool forEachLineCell(int x0, int y0, int x1, int y1, Visit&& visit) {
    const int ex = x1 >= x0 ? x1 - x0 : x0 - x1, ey = y1 >= y0 ? y1 - y0 : y0 - y1;
    const int sx = x1 >= x0 ? 1 : -1, sy = y1 >= y0 ? 1 : -1;
    const bool along_x = ex >= ey;
    const int long_ext = along_x ? ex : ey, short_ext = along_x ? ey : ex;
    int rem = long_ext / 2, x = x0, y = y0;
    for (int k = 0; k <= long_ext; ++k) {
      if (!visit(x, y)) return false;
      rem += short_ext;
      const bool side = rem >= long_ext;
      if (side) rem -= long_ext;
      x += along_x ? sx : (side ? sx : 0);
      y += along_x ? (side ? sy : 0) : sy;
    }
    return true;
  }
  // maximum cost over the line's cells, -1 as soon as one of them fails `fails(cost)`
  template <class Fails>
  __device__ double lineMax(int x0, int y0, int x1, int y1, Fails&& fails) const {
    double worst = 0.0;
    const bool clear = forEachLineCell(x0, y0, x1, y1, [&](int x, int y) {
      const uint8_t cost = master[(uint32_t)y * g.nx + (uint32_t)x];
      if (fails(cost)) return false;
      if (worst < (double)cost) worst = (double)cost;
      return true;
    });
    return clear ? worst : -1.0;
  }
  // CostmapModel::lineCost (costmap_model.cpp:104-125): a cell fails like pointCost
  __device__ double lineCost(int x0, int x1, int y0, int y1) const {
    return lineMax(x0, y0, x1, y1, [&](uint8_t cost) { return pointFails(cost); });
  }
  // the < 3 vertices branch of CostmapModel::footprintCost (:60-67): the centre cell alone, and INSCRIBED fails too
  __device__ double circularCost(uint32_t cell_x, uint32_t cell_y) const {
    const uint8_t cost = master[cell_y * g.nx + cell_x];
    if (cost == kLethal || cost == kInscribed || (cost == kNoInfo && !allow_unknown)) return -1.0;
    return cost;
  }
  // WorldModel::footprintCost(x, y, theta, spec) (world_model.h:65-86) + CostmapModel::footprintCost, one lane for all of it
  __device__ double footprintCost(double x, double y, double theta, const double* spec, uint32_t nfp) const {
    const double cos_th = cos(theta), sin_th = sin(theta);
    uint32_t cell_x, cell_y;
    if (!worldToMap(g, x, y, cell_x, cell_y)) return -1.0;
    if (nfp < 3) return circularCost(cell_x, cell_y);
    double footprint_cost = 0.0;
    uint32_t fx = 0, fy = 0, px = 0, py = 0;
    for (uint32_t v = 0; v <= nfp; ++v) {
      uint32_t vx, vy;
      if (v < nfp) {
        const double sx = spec[2 * v], sy = spec[2 * v + 1];
        const double wx = x + (sx * cos_th - sy * sin_th), wy = y + (sx * sin_th + sy * cos_th);
        if (!worldToMap(g, wx, wy, vx, vy)) return -1.0;
        if (v == 0) {
          fx = vx;
          fy = vy;
          px = vx;
          py = vy;
          continue;
        }
      } else {  // closing edge: last -> first
        vx = fx;
        vy = fy;
      }
      const double line_cost = lineCost((int)px, (int)vx, (int)py, (int)vy);
      footprint_cost = fmax(line_cost, footprint_cost);
      if (line_cost < 0) return -1.0;
      px = vx;
      py = vy;
    }
    return footprint_cost;
  }
};

}  // namespace navgpu
