// The rules of navfn::NavFn and of global_planner that more than one kernel of navfn_kernels.hip (or its host side) restates, once
// each, float / double arithmetic and narrowing points as the reference has them.  Arrays are read through a small functor the
// caller supplies, so a direct read (potarr[n]), a guarded one (potAt) and a read through an LDS window stay what they are at each
// call site: for the path walk the functor takes a cell OFFSET from the walker's cell stc, pot(ox, oy) = potarr[stc + ox + oy * nx].
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace navgpu {

constexpr float kPotHigh = 1.0e10f;      // POT_HIGH (navfn.h:77, global_planner/planner_core.h:48)
constexpr int kPriorityBufSize = 10000;  // PRIORITYBUFSIZE (navfn.h:80, dijkstra.h:47)
// `int minp = potarr[stc]` (navfn.cpp:895, gradient_path.cpp:119) with potarr[stc] == POT_HIGH is out of int range; the
// amd64 builds of the reference get cvttss2si's 0x80000000 there (so no neighbour is lower and the trace ends with "high
// potential"); v_cvt_i32_f32 would saturate to INT_MAX and walk on, so the amd64 value is restated.
__device__ __forceinline__ int truncX86(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000; }

// The two-neighbour interpolation (navfn.cpp:516-533, quadratic_calculator.cpp:60-76) from the lower horizontal neighbour tc,
// the lower vertical one ta and the cell's cost hf; the polynomial's literals are doubles, its value is narrowed before the product.
__device__ __forceinline__ float interpolatePotential(float tc, float ta, float hf) {
  float dc = tc - ta;
  if (dc < 0) {
    dc = -dc;
    ta = tc;
  }
  if (dc >= hf) return ta + hf;
  const float dd = dc / hf;  // (hf > 0 here: 0 <= dc < hf)
  const float v = (float)(-0.2301 * dd * dd + 0.5307 * dd + 0.7040);
  return ta + hf * v;
}

// DijkstraExpansion::getCost (dijkstra.h:78-87): whether a cell of raw cost `cost` is traversable, and its cost `c` if so.  What a
// cell that is not stands for is the caller's (lethal_cost for the expanders, "never updated" for the tiled wavefront).
__device__ __forceinline__ bool gpTraversableCost(uint8_t cost, int lethal, int neutral, float factor, bool unknown, float& c) {
  c = cost;
  if (c < lethal - 1 || (unknown && c == 255)) {
    c = c * factor + neutral;
    if (c >= lethal) c = lethal - 1;
    return true;
  }
  return false;
}

// The three priority buffers (navfn.h:160-170 push_cur / push_next / push_over, dijkstra.h:93-102): a cell is pushed once while
// its pending flag is up, and dropped when its buffer is full.  What makes a cell pushable differs (costarr[n] < COST_OBS for navfn,
// getCost(n) < lethal_cost for global_planner) and comes from the caller.
struct PriorityBuffers {
  int *cur, *next, *over;
  int cur_end = 0, next_end = 0, over_end = 0;
  uint8_t* pending;
  int ns;
  __device__ __forceinline__ PriorityBuffers(int* pb, uint8_t* pending_, int ns_)
      : cur(pb), next(pb + kPriorityBufSize), over(pb + 2 * kPriorityBufSize), pending(pending_), ns(ns_) {}
  template <class Pushable>
  __device__ __forceinline__ void push(int* buf, int& end, int n, Pushable pushable) {
    if (n >= 0 && n < ns && !pending[n] && pushable(n) && end < kPriorityBufSize) {
      buf[end++] = n;
      pending[n] = 1;
    }
  }
  template <class Pushable>
  __device__ __forceinline__ void pushCur(int n, Pushable pushable) { push(cur, cur_end, n, pushable); }
  // updateCell's tail (navfn.cpp:520-534, dijkstra.cpp:208-228): the neighbours whose potential l, r, u, d the new one undercuts by
  // more than their edge cost go to the next block when pot is below the threshold, to the overflow block otherwise
  template <class Pushable>
  __device__ __forceinline__ void pushNeighbours(bool low, int n, int nx, float pot, float l, float r, float u, float d, float le, float re, float ue,
                                                 float de, Pushable pushable) {
    int* buf = low ? next : over;
    int end = low ? next_end : over_end;
    if (l > pot + le) push(buf, end, n - 1, pushable);
    if (r > pot + re) push(buf, end, n + 1, pushable);
    if (u > pot + ue) push(buf, end, n - nx, pushable);
    if (d > pot + de) push(buf, end, n + nx, pushable);
    if (low) next_end = end; else over_end = end;
  }
  __device__ __forceinline__ void beginBlock() {
    for (int i = 0; i < cur_end; i++) pending[cur[i]] = 0;
  }
  // swap the priority blocks; with nothing left in the next one, raise the threshold and take the overflow block (navfn.cpp:671-689)
  __device__ __forceinline__ void endBlock(float& threshold, float increment) {
    cur_end = next_end;
    next_end = 0;
    int* pb = cur;
    cur = next;
    next = pb;
    if (cur_end == 0) {
      threshold += increment;
      cur_end = over_end;
      over_end = 0;
      pb = cur;
      cur = over;
      over = pb;
    }
  }
};

// ---- the path walk (NavFn::calcPath navfn.cpp:811-985, GradientPath::getPath gradient_path.cpp:68-248)
// gradCell (navfn.cpp:1001-1056, gradient_path.cpp:253-313) of the cell n = stc + qx + qy * nx, without its memo: false (and a zero
// gradient) for a cell of the border rows or with no slope.  The memo (gradx[n] + grady[n] > 0) stays with the callers: NavFn
// tests it before the bounds, GradientPath after them, which decides whether an out-of-range gradx[n] is read.  pot_nx1 is
// potarr[nx + 1], which the reference reads where potarr[n + nx] is meant (:1020, :287); obstacle is COST_OBS / lethal_cost.
template <class Pot>
__device__ __forceinline__ bool cellGradient(Pot pot, int qx, int qy, int n, int nx, int ns, float pot_nx1, float obstacle, float& gx, float& gy) {
  gx = gy = 0.0f;
  if (n < nx || n > ns - nx) return false;
  const float cv = pot(qx, qy);
  float dx = 0.0f, dy = 0.0f;
  if (cv >= kPotHigh) {
    if (pot(qx - 1, qy) < kPotHigh)
      dx = -obstacle;
    else if (pot(qx + 1, qy) < kPotHigh)
      dx = obstacle;
    if (pot(qx, qy - 1) < kPotHigh)
      dy = -obstacle;
    else if (pot_nx1 < kPotHigh)
      dy = obstacle;
  } else {
    if (pot(qx - 1, qy) < kPotHigh) dx += pot(qx - 1, qy) - cv;
    if (pot(qx + 1, qy) < kPotHigh) dx += cv - pot(qx + 1, qy);
    if (pot(qx, qy - 1) < kPotHigh) dy += pot(qx, qy - 1) - cv;
    if (pot(qx, qy + 1) < kPotHigh) dy += cv - pot(qx, qy + 1);
  }
  float norm = (float)hypot((double)dx, (double)dy);
  if (!(norm > 0)) return false;
  norm = (float)(1.0 / norm);
  gx = norm * dx;
  gy = norm * dy;
  return true;
}

// "check for potentials at eight positions near cell" (navfn.cpp:872-881): the walker stands on a boundary of the potential function
template <class Pot>
__device__ __forceinline__ bool highAmongNine(Pot pot) {
  return pot(0, 0) >= kPotHigh || pot(1, 0) >= kPotHigh || pot(-1, 0) >= kPotHigh || pot(0, 1) >= kPotHigh || pot(1, 1) >= kPotHigh ||
         pot(-1, 1) >= kPotHigh || pot(0, -1) >= kPotHigh || pot(1, -1) >= kPotHigh || pot(-1, -1) >= kPotHigh;
}

// The grid step (navfn.cpp:893-925, gradient_path.cpp:117-146): the offset of the lowest of the eight neighbours, (0, 0) if none is
// lower.  minp is an int in the reference: the centre through truncX86, each neighbour accepted through a plain (int).
template <class Pot>
__device__ __forceinline__ void lowestOfEight(Pot pot, int& mox, int& moy) {
  mox = moy = 0;
  int minp = truncX86(pot(0, 0));
  const int ox[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, oy[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float v = pot(ox[q], oy[q]);
    if (v < (float)minp) {
      minp = (int)v;
      mox = ox[q];
      moy = oy[q];
    }
  }
}

// The gradient step (navfn.cpp:944-977, gradient_path.cpp:201-238): the gradients g[0..3] of stc, stc + 1, stc + nx, stc + nx + 1
// interpolated bilinearly at (dx, dy), a step of pathStep (0.5) along the result, and the carries into the cell index.  false = zero
// gradient, nothing moved.
__device__ __forceinline__ bool gradientStep(const float (&gx)[4], const float (&gy)[4], int nx, int& stc, float& dx, float& dy) {
  const float x1 = (float)((1.0 - dx) * gx[0] + dx * gx[1]);
  const float x2 = (float)((1.0 - dx) * gx[2] + dx * gx[3]);
  const float x = (float)((1.0 - dy) * x1 + dy * x2);
  const float y1 = (float)((1.0 - dx) * gy[0] + dx * gy[1]);
  const float y2 = (float)((1.0 - dx) * gy[2] + dx * gy[3]);
  const float y = (float)((1.0 - dy) * y1 + dy * y2);
  if (x == 0.0 && y == 0.0) return false;
  const float ss = (float)(0.5f / hypot((double)x, (double)y));
  dx += x * ss;
  dy += y * ss;
  if (dx > 1.0) { stc++; dx = (float)(dx - 1.0); }
  if (dx < -1.0) { stc--; dx = (float)(dx + 1.0); }
  if (dy > 1.0) { stc += nx; dy = (float)(dy - 1.0); }
  if (dy < -1.0) { stc -= nx; dy = (float)(dy + 1.0); }
  return true;
}

// DijkstraExpansion::setPreciseStart's seeds (planner_core.cpp:124-127, dijkstra.cpp:88-103): the four cells round the start and the
// potentials they begin with, the start's sub-cell offset rounded to a hundredth
__host__ __device__ inline void preciseStartSeeds(double start_x, double start_y, int nx, int neutral, int (&cells)[4], float (&vals)[4]) {
  const int k = (int)start_x + nx * (int)start_y;
  double dx = start_x - (int)start_x, dy = start_y - (int)start_y;
  dx = floorf((float)(dx * 100 + 0.5)) / 100;
  dy = floorf((float)(dy * 100 + 0.5)) / 100;
  cells[0] = k;
  cells[1] = k + 1;
  cells[2] = k + nx;
  cells[3] = k + nx + 1;
  vals[0] = (float)(neutral * 2 * dx * dy);
  vals[1] = (float)(neutral * 2 * (1 - dx) * dy);
  vals[2] = (float)(neutral * 2 * dx * (1 - dy));
  vals[3] = (float)(neutral * 2 * (1 - dx) * (1 - dy));
}

}  // namespace navgpu
