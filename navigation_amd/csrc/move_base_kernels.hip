// move_base's planner-side executive for a fleet (move_base/src/move_base.cpp), the device side:
//   k_plan_prefer        MoveBase::preferPrevPlan + findClosestPlanIndex (:784-836) on the resident controller plans, and the
//                        predicate of the adoption's emit kernel
//   k_set_polygon_cost   Costmap2D::setConvexPolygonCost (costmap_2d.cpp:315-428) on the master or the obstacle grid, for
//                        MoveBase::clearCostmapWindows (:277-330) and MoveSlowAndClear::runBehavior (move_slow_and_clear.cpp:83-127)
// gfx950, wave64.  fp64 as written in the reference, uncontracted (-ffp-contract=off).  No atomics between workgroups, and within
// one only integer minima / maxima in LDS: the results are a function of the inputs alone.
#include <limits.h>

#include "navgpu_device.h"

namespace navgpu {

constexpr int kPpWaves = kPlanPreferThreads / 64;
constexpr int kPpNone = INT_MAX;

// hypot(x, y) as move_base's distance() calls it (:778-782).  libm's is not correctly rounded, so its bits cannot be restated; this
// is hyp2's compensated sqrt(x * x + y * y) (within 1 ulp of the true value, as libm's is) on operands scaled by a power of two,
// which keeps the squares in range, and with the larger magnitude first, which makes it symmetric in its arguments: equal distances
// by construction (a mirrored pose) compare equal here as they do on the host.  NaN in, NaN out: it then fails `dist < min_dist`.
__device__ __forceinline__ double ppHypot(double x, double y) {
  double a = fabs(x), b = fabs(y);
  if (a < b) {
    const double t = a;
    a = b;
    b = t;
  }
  if (!(a < __builtin_inf()) || a == 0.0) return a + b;  // an infinity, a NaN (either operand), or both zero
  const int e = ilogb(a);
  return ldexp(hyp2(ldexp(a, -e), ldexp(b, -e)), e);
}

// One workgroup per robot.  findClosestPlanIndex's loop (`if (dist < min_dist)` from min_dist = 1e9 over i = 0, 4, 8, ...) picks
// the first index of the strictly smallest distance below 1e9: every lane keeps that of the samples it visits, a chunk of
// kPlanPreferThreads samples at a time in ascending order, and the lanes' answers are reduced by (distance, index) - through the
// waves' shuffles, then one LDS word pair per wave.
__global__ __launch_bounds__(kPlanPreferThreads) void k_plan_prefer(const navgpu_global_pose* store, uint32_t max_global_plan, uint32_t first,
                                                                    const PlanPreferIn* in, int64_t* persistence, int64_t now_ns,
                                                                    int64_t timeout_ns, navgpu_handover_record* rec, uint32_t* emit_off) {
  __shared__ double wave_d[kPpWaves];
  __shared__ int wave_i[kPpWaves];
  const uint32_t inst = first + blockIdx.x, tid = threadIdx.x;
  const PlanPreferIn a = in[blockIdx.x];
  if (!(a.flags & kPpActive)) {  // (the whole workgroup) the host has written the record of a plan that was not made or is too long
    if (tid == 0) emit_off[blockIdx.x] = kPpNoWrite;
    return;
  }
  const navgpu_global_pose* p = store + (size_t)inst * max_global_plan;
  const uint64_t orig_len = (uint64_t)a.dropped + a.stored;  // controller_plan_->size()
  double my_d = __builtin_inf();
  int my_i = kPpNone;
  // original indices i = 0 (mod 4), i >= dropped; slot position i - dropped
  for (uint64_t i = 4 * (((uint64_t)a.dropped + 3) / 4 + tid); i < orig_len; i += 4 * (uint64_t)kPlanPreferThreads) {
    const navgpu_global_pose q = p[i - a.dropped];
    const double d = ppHypot(a.x - q.x, a.y - q.y);
    if (d < 1000000000.0 && d < my_d) {
      my_d = d;
      my_i = (int)i;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double od = __shfl_xor(my_d, off, 64);
    const int oi = __shfl_xor(my_i, off, 64);
    if (od < my_d || (od == my_d && oi < my_i)) {
      my_d = od;
      my_i = oi;
    }
  }
  if ((tid & 63) == 0) {
    wave_d[tid >> 6] = my_d;
    wave_i[tid >> 6] = my_i;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < kPpWaves; ++w)
    if (wave_d[w] < my_d || (wave_d[w] == my_d && wave_i[w] < my_i)) {
      my_d = wave_d[w];
      my_i = wave_i[w];
    }
  const uint64_t closest_i = my_i == kPpNone ? 0 : (uint64_t)my_i;
  const uint64_t prev_len = orig_len - closest_i;
  const bool prefer_prev = prev_len + 320 < (uint64_t)a.new_len;
  int64_t state = persistence[inst];
  bool keep = false;
  if (prefer_prev && state != NAVGPU_PERSISTENCE_INITIAL) {  // move_base.cpp:815-830
    if (state == NAVGPU_PERSISTENCE_NEWPLAN) state = now_ns + timeout_ns;
    keep = now_ns < state;
  }
  if (!keep) state = NAVGPU_PERSISTENCE_NEWPLAN;  // :831
  persistence[inst] = state;
  emit_off[blockIdx.x] = keep ? kPpNoWrite : inst * max_global_plan;  // (n * max_global_plan <= 2^32 - 1: navgpu_local_planner_reserve_plans)
  navgpu_handover_record r{};
  r.decision = keep ? NAVGPU_HANDOVER_KEEP : NAVGPU_HANDOVER_ADOPT;
  r.closest_index = (int32_t)closest_i;
  r.prev_len = (int32_t)prev_len;
  r.new_len = (int32_t)a.new_len;
  r.dropped = (int32_t)a.dropped;
  r.persistence_end_ns = state;
  rec[blockIdx.x] = r;
}

// One 256-thread workgroup per robot: a vertex per lane through worldToMap, an outline edge per lane through raytraceLine into the
// columns' lowest and highest outline cell (integer minima / maxima in LDS: order-free), then the fill goes row by row, a lane per
// column.  The columns are taken kPolyCols at a time, so a polygon may span the whole map; every chunk walks the outline again and keeps what
// falls into it.  The rule - per column, everything between the lowest and the highest outline cell - is k_obstacle's
// clearFootprintPolygon (costmap_kernels.hip), which states why it equals convexFillCells.
constexpr uint32_t kPolyCols = 1024;
__global__ __launch_bounds__(256) void k_set_polygon_cost(CostmapDev cm, uint8_t* grid, uint32_t first, const double* xy, const uint32_t* off,
                                                          uint8_t value, int32_t* ok_out) {
  __shared__ uint32_t s_vx[NAVGPU_MAX_POLYGON], s_vy[NAVGPU_MAX_POLYGON];
  __shared__ uint32_t colmin[kPolyCols], colmax[kPolyCols];
  __shared__ int s_ok;
  const uint32_t inst = first + blockIdx.x, tid = threadIdx.x;
  const Geom g{cm.origin[2 * inst], cm.origin[2 * inst + 1], cm.res, cm.nx, cm.ny};
  const uint32_t at = off[blockIdx.x];
  const uint32_t n = min(off[blockIdx.x + 1] - at, (uint32_t)NAVGPU_MAX_POLYGON);  // (the host has refused more)
  if (tid == 0) s_ok = 1;
  __syncthreads();
  for (uint32_t v = tid; v < n; v += blockDim.x) {
    uint32_t mx = 0, my = 0;
    const bool ok = worldToMap(g, xy[2 * (size_t)(at + v)], xy[2 * (size_t)(at + v) + 1], mx, my);
    s_vx[v] = mx;
    s_vy[v] = my;
    if (!ok) atomicAnd(&s_ok, 0);
  }
  __syncthreads();
  const int ok = s_ok;
  if (tid == 0) ok_out[blockIdx.x] = ok;
  if (!ok || n < 3) return;  // (the whole workgroup) :323-324; convexFillCells' "we need a minimum polygon of a triangle" (:383-384)
  uint32_t minx = 0xFFFFFFFFu, maxx = 0, miny = 0xFFFFFFFFu, maxy = 0;  // (an outline cell lies inside the vertices' box)
  for (uint32_t i = 0; i < n; ++i) {
    minx = s_vx[i] < minx ? s_vx[i] : minx;
    maxx = s_vx[i] > maxx ? s_vx[i] : maxx;
    miny = s_vy[i] < miny ? s_vy[i] : miny;
    maxy = s_vy[i] > maxy ? s_vy[i] : maxy;
  }
  uint8_t* cells = grid + (size_t)inst * cm.cells_padded;
  for (uint32_t c0 = minx; c0 <= maxx; c0 += kPolyCols) {  // (maxx < nx < 2^31: no wrap)
    const uint32_t span = min(kPolyCols, maxx - c0 + 1);
    for (uint32_t c = tid; c < span; c += blockDim.x) {
      colmin[c] = 0xFFFFFFFFu;
      colmax[c] = 0;
    }
    __syncthreads();
    for (uint32_t v = tid; v < n; v += blockDim.x) {
      const uint32_t e1 = (v + 1 == n) ? 0 : v + 1;  // the last edge closes the outline (:359-363)
      raytrace2d(g.nx, s_vx[v], s_vy[v], s_vx[e1], s_vy[e1], 0xFFFFFFFFu, [&](uint32_t cell) {
        const uint32_t y = cell / g.nx, x = cell - y * g.nx;
        if (x >= c0 && x - c0 < span) {
          atomicMin(&colmin[x - c0], y);
          atomicMax(&colmax[x - c0], y);
        }
      });
    }
    __syncthreads();
    // the fill, row by row with a lane per column: a wave's stores of one row are neighbouring bytes
    for (uint32_t c = tid; c < span; c += blockDim.x) {
      const uint32_t lo = colmin[c], hi = colmax[c];
      for (uint32_t y = miny; y <= maxy; ++y)
        if (lo <= y && y <= hi) cells[(size_t)y * g.nx + c0 + c] = value;  // (lo = 0xFFFFFFFF, hi = 0: a column without outline cells)
    }
    __syncthreads();  // (colmin / colmax are written again by the next chunk)
  }
}

void launch_plan_prefer(const navgpu_global_pose* store, uint32_t max_global_plan, uint32_t first, uint32_t count, const PlanPreferIn* in,
                        int64_t* persistence, int64_t now_ns, int64_t timeout_ns, navgpu_handover_record* rec, uint32_t* emit_off, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_prefer, dim3(count), dim3(kPlanPreferThreads), 0, s, store, max_global_plan, first, in, persistence, now_ns, timeout_ns,
                     rec, emit_off);
}
void launch_set_polygon_cost(const CostmapDev& cm, uint8_t* grid, uint32_t first, uint32_t count, const double* xy, const uint32_t* off,
                             uint8_t value, int32_t* ok, hipStream_t s) {
  hipLaunchKernelGGL(k_set_polygon_cost, dim3(count), dim3(256), 0, s, cm, grid, first, xy, off, value, ok);
}

}  // namespace navgpu
