// NavFn::calcPath on one lane, shared by k_navfn_plan (navfn_kernels.hip) and k_nr_path (navfn_ros_kernels.hip).
#pragma once
#include "navfn_rules.h"
#include "navgpu_device.h"

namespace navgpu {

constexpr int kCostObs = 254, kCostNeutral = 50;  // COST_OBS, COST_NEUTRAL (navfn.h:49-67)

// NavFn::calcPath / gradCell (navfn.cpp:811-1056) over one plan's potential array, one lane: the interpolated gradient descent from the
// start cell, its result record included (the tiled wavefront's walk by one wave is k_navfn_wf_path).
__device__ inline void navfnCalcPath(const NavfnDev& nv, uint32_t plan, const float* potarr, int goal0, int goal1, int start0, int start1, int n_max,
                              int cycle) {
  const int nx = nv.nx, ny = nv.ny, ns = nv.ns;
  float* gradx = nv.gradx + (size_t)plan * nv.ns_padded;
  float* grady = nv.grady + (size_t)plan * nv.ns_padded;
  float* pathx = nv.path + (size_t)plan * 2 * nv.path_cap;
  float* pathy = pathx + nv.path_cap;
  const int startCell = start1 * nx + start0;
  const float pot_nx1 = potarr[nx + 1];
  int stc = startCell, npath = 0, found = 0;
  float dx = 0, dy = 0;
  auto pot = [&](int ox, int oy) -> float { return potarr[stc + ox + oy * nx]; };
  auto gradCell = [&](int qx, int qy) {  // NavFn tests the memo first: gradx[n] is read for whichever n the walker asks
    const int n = stc + qx + qy * nx;
    if (gradx[n] + grady[n] > 0.0) return;
    float gx, gy;
    if (cellGradient(pot, qx, qy, n, nx, ns, pot_nx1, (float)kCostObs, gx, gy)) {
      gradx[n] = gx;
      grady[n] = gy;
    }
  };
  for (int i = 0; i < n_max && i < (int)nv.path_cap; i++) {  // (NavFn's walk stops at the buffer's end; GradientPath's counts on)
    const int nearest_point = max(0, min(nx * ny - 1, stc + (int)round((double)dx) + (int)(nx * round((double)dy))));
    if (potarr[nearest_point] < (float)kCostNeutral) {  // NavFn's end test: a potential below COST_NEUTRAL is the goal's
      pathx[npath] = (float)goal0;
      pathy[npath] = (float)goal1;
      ++npath;
      found = 1;
      break;
    }
    if (stc < nx || stc > ns - nx) break;  // would be out of bounds
    pathx[npath] = (float)(stc % nx) + dx;
    pathy[npath] = (float)(stc / nx) + dy;
    npath++;
    const bool oscillation_detected = npath > 2 && pathx[npath - 1] == pathx[npath - 3] && pathy[npath - 1] == pathy[npath - 3];
    if (highAmongNine(pot) || oscillation_detected) {
      int mox, moy;
      lowestOfEight(pot, mox, moy);
      stc += mox + moy * nx;
      dx = 0;
      dy = 0;
      if (potarr[stc] >= kPotHigh) break;
    } else {
      gradCell(0, 0);
      gradCell(1, 0);
      gradCell(0, 1);
      gradCell(1, 1);
      const int stcnx = stc + nx;
      const float gx[4] = {gradx[stc], gradx[stc + 1], gradx[stcnx], gradx[stcnx + 1]};
      const float gy[4] = {grady[stc], grady[stc + 1], grady[stcnx], grady[stcnx + 1]};
      if (!gradientStep(gx, gy, nx, stc, dx, dy)) break;  // zero gradient
    }
  }
  navgpu_navfn_result r;
  r.found = found;
  r.path_length = found ? npath : 0;
  r.cycles = cycle;
  r.start_potential = potarr[startCell];
  nv.results[plan] = r;
}

}  // namespace navgpu
