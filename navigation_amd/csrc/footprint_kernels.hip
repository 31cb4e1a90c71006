// HIP kernel (gfx950) behind navgpu_footprint_cost, navgpu_rotate_recovery_step and navgpu_carrot_plan:
//   k_footprint_cost : WorldModel::footprintCost(x, y, theta, spec) -> CostmapModel::footprintCost (world_model.h:65-86,
//                      costmap_model.cpp:50-142) for a run of poses per robot, against the robot's resident footprint, master
//                      grid and origin.
// The answer is order-free - a maximum over the outline's cells, and every failure yields the same -1 - so a lane takes one
// (query, edge) task, the closing edge among them: a workgroup holds 256 / n_vertices whole queries of one robot,
//   pass 0  one lane per query : centre cell, cos / sin of the heading (fp64) into LDS; robots with < 3 vertices end here
//   pass 1  one lane per vertex: x + (sx * cos - sy * sin), worldToMap, the cell into LDS
//   pass 2  one lane per edge  : the reference's LineIterator walk from its vertex to the next, atomicMax into the query's LDS word
//   pass 3  one lane per query : the double, and atomicMin of the first failing (or first legal) query of the robot
// A query's edges may straddle waves, a robot's queries straddle workgroups.  -DNAVGPU_FOOTPRINT_LANE_PER_QUERY (tools/
// bench_footprint_cost.py only) builds the other split, one lane per query walking the whole outline, for comparison.
// Compiled with -ffp-contract=off.
#include <algorithm>

#include "costmap_model_dev.h"

namespace navgpu {

constexpr uint32_t kFpThreads = 256;
constexpr uint32_t kFpFail = 0xFFFFFFFFu;  // LDS word of a query: 0..255 the largest cost so far, kFpFail = -1.0; also "vertex off the map"
#ifdef NAVGPU_FOOTPRINT_LANE_PER_QUERY
constexpr bool kFpLanePerQuery = true;
#else
constexpr bool kFpLanePerQuery = false;
#endif
static_assert(kMaxFootprint <= (int)kFpThreads, "a workgroup holds at least one whole query");

// lanes a query of a robot with nfp vertices takes (host and device agree on the launch shape through this)
__host__ __device__ inline uint32_t fpLanesPerQuery(uint32_t nfp) { return (kFpLanePerQuery || nfp < 3) ? 1u : nfp; }

__global__ __launch_bounds__(kFpThreads) void k_footprint_cost(FootprintDev d, uint32_t first) {
  const uint32_t k = blockIdx.y, inst = first + k;
  const uint32_t q0 = d.q_off[k], nq = d.q_off[k + 1] - q0;
  const uint32_t nfp = min(d.fp_n[inst], (uint32_t)kMaxFootprint);
  const uint32_t E = fpLanesPerQuery(nfp);
  const uint32_t per_block = kFpThreads / E;
  const uint32_t base = blockIdx.x * per_block;
  if (base >= nq) return;  // (the whole workgroup: the grid is sized for the longest run of the launch)
  const uint32_t here = min(per_block, nq - base);
  __shared__ double s_cos[kFpThreads], s_sin[kFpThreads];
  __shared__ uint32_t s_word[kFpThreads], s_vert[kFpThreads];
  CostmapModelDev wm;
  wm.master = d.master + (size_t)inst * d.cells_padded;
  wm.g = Geom{d.origin[2 * inst], d.origin[2 * inst + 1], d.res, d.nx, d.ny};
  wm.allow_unknown = d.allow_unknown != 0;
  const double* spec = d.fp_spec + (size_t)inst * kMaxFootprint * 2;
  const uint32_t t = threadIdx.x;
  const bool split = E > 1;

  if (t < here) {  // pass 0
    const double* p = d.poses + (size_t)(q0 + base + t) * 3;
    uint32_t word = 0;
    if (!split) {
      const double c = wm.footprintCost(p[0], p[1], p[2], spec, nfp);
      word = c < 0 ? kFpFail : (uint32_t)c;
    } else {
      uint32_t cell_x, cell_y;
      if (!worldToMap(wm.g, p[0], p[1], cell_x, cell_y)) word = kFpFail;
      s_cos[t] = cos(p[2]);
      s_sin[t] = sin(p[2]);
    }
    s_word[t] = word;
  }
  if (split) {
    __syncthreads();
    const uint32_t lq = t / E, e = t - lq * E;
    const bool live = lq < here && s_word[lq] != kFpFail;
    if (live) {  // pass 1
      const double* p = d.poses + (size_t)(q0 + base + lq) * 3;
      const double cos_th = s_cos[lq], sin_th = s_sin[lq];
      const double sx = spec[2 * e], sy = spec[2 * e + 1];
      const double wx = p[0] + (sx * cos_th - sy * sin_th), wy = p[1] + (sx * sin_th + sy * cos_th);
      uint32_t vx, vy;
      s_vert[t] = worldToMap(wm.g, wx, wy, vx, vy) ? (vx | (vy << 16)) : kFpFail;  // size_x, size_y <= 65535 (navgpu_fleet_create)
    }
    __syncthreads();
    if (live) {  // pass 2
      const uint32_t a = s_vert[t], b = s_vert[lq * E + (e + 1 == E ? 0 : e + 1)];
      uint32_t r = kFpFail;
      if (a != kFpFail && b != kFpFail) {
        const double line_cost = wm.lineCost((int)(a & 0xFFFFu), (int)(b & 0xFFFFu), (int)(a >> 16), (int)(b >> 16));
        r = line_cost < 0 ? kFpFail : (uint32_t)line_cost;
      }
      if (r) atomicMax(&s_word[lq], r);
    }
    __syncthreads();
  }
  if (t < here) {  // pass 3
    const uint32_t word = s_word[t];
    const double cost = word == kFpFail ? -1.0 : (double)word;
    d.costs[q0 + base + t] = cost;
    if (d.first_hit && (cost < 0) != (d.seek_legal != 0)) atomicMin(&d.first_hit[k], base + t);
  }
}

// h_counts = the `count` run lengths, h_fp_n = the fleet's vertex counts (absolute instance)
void launch_footprint_cost(const FootprintDev& d, uint32_t first, uint32_t count, const uint32_t* h_counts, const uint32_t* h_fp_n, hipStream_t s) {
  uint32_t blocks = 0;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t per_block = kFpThreads / fpLanesPerQuery(std::min<uint32_t>(h_fp_n[first + k], kMaxFootprint));
    blocks = std::max(blocks, (h_counts[k] + per_block - 1) / per_block);
  }
  if (blocks == 0) return;
  hipLaunchKernelGGL(k_footprint_cost, dim3(blocks, count), dim3(kFpThreads), 0, s, d, first);
}

}  // namespace navgpu
