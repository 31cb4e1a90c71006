// Shared by planner_score.hip (the general k_score kernels and the per-robot image k_score_prep* builds) and
// planner_score_sweep.hip (the product kernel k_score_sweep, which loads that image).
#pragma once
#include "planner_common.h"

namespace navgpu {

// The tables (use_tables: use_dwa && discretize_by_time, k_score_prep_tab only): the heading sequence theta_k of a sample
// depends only on its v_theta and the step (theta += v_theta*dt, rounded to float each step), so sincos(theta_k),
// sincos(pi/2+theta_k) and the rotated footprint vertices are computed once per (v_theta sample, step) into the robot's
// image, and k_score_sweep shares them among all (vx, vy) samples.  The arithmetic per value is unchanged (same
// operations, same rounding), only deduplicated.
__host__ __device__ inline size_t score_bits_bytes(int win) {  // [win][nw][4] words (part of the LDS image), 16-byte aligned
  return (((size_t)4 * win * ((win + 31) >> 5) * 4) + 15) & ~(size_t)15;
}
// the two [win][nw][2] word arrays the dilation passes work in: behind the image, only where the image is BUILT (buildScreens)
__host__ __device__ inline size_t score_scratch_bytes(int win) { return score_bits_bytes(win); }
// CHUNK: cells of a footprint edge fetched per LDS round trip; the launcher picks the smallest of 6 / 9 / 12 / 16 that
// covers the longest edge (a 0.4 m square at 0.05 m: 9), longer edges take several chunks
// AGG: the MapGridCostFunction options DWAPlanner itself never sets - aggregation Sum / Product and a sideways shift
// (map_grid_cost_function.cpp:75-129) - as navgpu_planner_set_map_grid_options configures them: every live critic looks
// its own cell up at every point (no screen, no shared cell); the product kernels are compiled without it.
// n / d for 0 <= n < 2^22, 1 <= d < 2^22: float quotient + one correction step either way (the generic 32-bit division is
// ~40 vector instructions, and every lane of a scoring workgroup makes two of them)
__device__ __forceinline__ int divSmall(int n, int d) {
  int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
  int r = n - q * d;
  if (r < 0) {
    --q;
    r += d;
  }
  if (r >= d) ++q;
  return q;
}

// Costmap2D::worldToMap (costmap_2d.cpp:208-220) with the two fp64 divisions replaced by a multiply; exact: whenever the
// product is not clear of an integer by 1e-7 (error bound 5e-10 below 1e6 cells) the division is redone.
// Straight-line: the only branch is the rare redo.  Bound to the kernel's locals by reference, as the lambda it replaces
// captured them (passed as values, the kernels compile to a different, equivalent instruction order).
struct WorldToMapFast {
  const Geom& g;
  const double& inv_res;
  __device__ __forceinline__ bool operator()(double wx, double wy, uint32_t& mx, uint32_t& my) const {
    const double dx = wx - g.ox, dy = wy - g.oy;
    const double qx = dx * inv_res, qy = dy * inv_res;
    double fx = floor(qx), fy = floor(qy);
    const double rx = qx - fx, ry = qy - fy;
    if (__builtin_expect(fmin(rx, ry) < 1.0e-7 || fmax(rx, ry) > 1.0 - 1.0e-7, 0)) {
      fx = !(dx >= 0.0) ? -1.0 : (qx >= 1.0e6 ? 1.0e6 : (double)(int)(dx / g.res));  // wx < origin -> false (costmap_2d.cpp:210)
      fy = !(dy >= 0.0) ? -1.0 : (qy >= 1.0e6 ? 1.0e6 : (double)(int)(dy / g.res));
    }
    // v_cvt_i32_f64 saturates (a point left of / below the origin floors to a negative cell, one far beyond the grid to
    // INT_MAX: both fail the size test as unsigned numbers), which a C++ cast does not promise
    int ix, iy;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(ix) : "v"(fx));
    asm("v_cvt_i32_f64 %0, %1" : "=v"(iy) : "v"(fy));
    mx = (uint32_t)ix;
    my = (uint32_t)iy;
    return mx < g.nx && my < g.ny;
  }
};

// one critic's term of scoreTrajectory's sum (simple_scored_sampling_planner.cpp:59-75), added in DWAPlanner's critic order
// (dwa_planner.cpp:167-173) by the caller: a critic that is off (scale 0) adds nothing, a cost of 0 is not scaled
__device__ __forceinline__ void addCritic(double& total, bool en, double value, double scale) {
  if (!en) return;
  double cost = value;
  if (cost != 0) cost *= scale;
  total += cost;
}

// behind a robot's image in pl.prep (k_score_prep_tab writes them, k_score_sweep reads them): kScoreAuxBytes of per-robot scalars
// and one byte per (vx, vy) pair, at the END of the robot's slot
constexpr uint32_t kScoreAuxBytes = 64;
__host__ __device__ inline uint32_t score_prep_reject_bytes(const PlannerDev& pl) { return (pl.max_axis * pl.max_axis + 255u) & ~255u; }
__host__ __device__ inline uint32_t score_prep_reject_offset(const PlannerDev& pl) { return pl.prep_stride - score_prep_reject_bytes(pl); }
// a scoring launch with `lds` bytes of dynamic LDS, allowed for the kernel first when there are more than kAllowAbove
template <size_t kAllowAbove = 48 * 1024, typename... P, typename... A>
void launchScore(void (*kernel)(P...), dim3 grid, int threads, size_t lds, hipStream_t s, A... args) {
  if (lds > kAllowAbove) hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, args...);
}
size_t score_table_row_bytes(const PlannerDev& pl);
size_t score_table_lds_bytes(const PlannerDev& pl);
// k_score_sweep (planner_score_sweep.hip): the launch for use_tables with DWAPlanner's own MapGrid options
bool score_sweep_applies(const PlannerDev& pl);
uint32_t launch_score_sweep(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s);  // returns blocks per instance
uint32_t launch_score_sweep_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s);  // the same for a robot list

}  // namespace navgpu
