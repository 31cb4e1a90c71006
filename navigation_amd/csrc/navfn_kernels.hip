// navfn::NavFn on the device: the potential-field expansion behind the navfn / global_planner global
// planners and the gradient-descent path extraction, for a batch of independent plans.
//   NavFn::setCostmap (navfn/src/navfn.cpp:222-283)           k_navfn_costmap   one thread per cell
//   NavFn::setupNavFn / initCost (:379-453)                    k_navfn_plan, all lanes
//   NavFn::propNavFnDijkstra / updateCell (:466-535, 633-701)  k_navfn_plan, lane 0
//   NavFn::propNavFnAstar / updateCellAstar (:548-620, 714-791)
//   NavFn::calcPath / gradCell (:811-1056)
// The expansion is not a Dijkstra proper: cells are relaxed out of three priority buffers in buffer order, a cell sees
// the potentials its predecessors IN THE SAME BLOCK have just written, the buffers hold 10 000 entries and drop what does
// not fit, and the search stops the moment the start cell has a potential - the array it leaves is a snapshot of a
// sequential process, final near the path and provisional elsewhere.  A wavefront that relaxes a block in
// parallel computes a different array.  What is reproduced here is therefore the process itself: one lane per plan walks
// the buffers in the reference's order with the reference's float/double arithmetic, bit for bit, while the other lanes of
// its wave only initialise the arrays; the batch dimension (one plan per robot of a fleet, 256 at a time on 256 CUs, the
// costmaps already resident in HBM) is where the device is used.
#include <hip/hip_runtime.h>

#include "navfn_calc_path.h"
#include "navfn_rules.h"
#include "navgpu_device.h"

namespace navgpu {

namespace {
constexpr int kCostUnknownRos = 255, kCostObsRos = 253;  // navfn.h:49-67 (COST_OBS and COST_NEUTRAL: navfn_calc_path.h)
}  // namespace

// NavFn::setCostmap: cost_mode 0 = the bytes ARE costarr, 1 = isROS, 2 = plain PGM (borders of 7 cells stay obstacles)
__global__ __launch_bounds__(256) void k_navfn_costmap(NavfnDev nv, uint32_t first, const uint8_t* cmap, size_t cmap_stride, int cost_mode,
                                                       int allow_unknown) {
  const uint32_t plan = first + blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= nv.ns) return;
  const uint8_t in = cmap[(size_t)blockIdx.y * cmap_stride + n];
  uint8_t out = (uint8_t)kCostObs;
  if (cost_mode == 0) {
    out = in;
  } else {
    const int i = n / nv.nx, j = n - i * nv.nx;
    const bool border = cost_mode == 2 && (i < 7 || i > nv.ny - 8 || j < 7 || j > nv.nx - 8);
    if (!border) {
      int v = in;
      if (v < kCostObsRos) {
        v = (int)(kCostNeutral + 0.8 * v);  // COST_NEUTRAL + COST_FACTOR * v, in double, truncated (:238)
        if (v >= kCostObs) v = kCostObs - 1;
        out = (uint8_t)v;
      } else if (v == kCostUnknownRos && (allow_unknown || cost_mode == 2)) {
        out = (uint8_t)(kCostObs - 1);
      }
    }
  }
  nv.costarr[(size_t)plan * nv.ns_padded + n] = out;
}

// setupNavFn(keepit = true) (:379-440), all lanes of the block
__device__ __forceinline__ void navfnSetup(const NavfnDev& nv, uint32_t plan) {
  const int nx = nv.nx, ny = nv.ny;
  const size_t base = (size_t)plan * nv.ns_padded;
  for (int i = threadIdx.x; i < nv.ns; i += blockDim.x) {
    nv.potarr[base + i] = kPotHigh;
    nv.gradx[base + i] = 0.0f;
    nv.grady[base + i] = 0.0f;
    nv.pending[base + i] = 0;
    const int y = i / nx, x = i - y * nx;
    if (y == 0 || y == ny - 1 || x == 0 || x == nx - 1) nv.costarr[base + i] = (uint8_t)kCostObs;  // outer bounds of the cost array
  }
  __syncthreads();
}

// initCost (:445-453), then propNavFnDijkstra / propNavFnAstar over updateCell / updateCellAstar (:466-791), one lane: the cycles used
__device__ int navfnPropagate(const NavfnDev& nv, uint32_t plan, int goal0, int goal1, int start0, int start1, int astar, int at_start) {
  const int nx = nv.nx, ny = nv.ny;
  const uint8_t* costarr = nv.costarr + (size_t)plan * nv.ns_padded;
  float* potarr = nv.potarr + (size_t)plan * nv.ns_padded;
  PriorityBuffers pb(nv.pb + (size_t)plan * 3 * kPriorityBufSize, nv.pending + (size_t)plan * nv.ns_padded, nv.ns);
  float curT = (float)kCostObs;
  const float priInc = 2 * kCostNeutral;
  auto pushable = [&](int n) { return costarr[n] < kCostObs; };
  {
    const int k = goal0 + goal1 * nx;
    potarr[k] = 0.0f;
    pb.pushCur(k + 1, pushable);
    pb.pushCur(k - 1, pushable);
    pb.pushCur(k - nx, pushable);
    pb.pushCur(k + nx, pushable);
  }
  auto updateCell = [&](int n) {
    const float l = potarr[n - 1], r = potarr[n + 1], u = potarr[n - nx], d = potarr[n + nx];
    if (costarr[n] >= kCostObs) return;  // don't propagate into obstacles
    float pot = interpolatePotential(l < r ? l : r, u < d ? u : d, (float)costarr[n]);
    if (pot < potarr[n]) {
      const float le = (float)(0.707106781 * (float)costarr[n - 1]);
      const float re = (float)(0.707106781 * (float)costarr[n + 1]);
      const float ue = (float)(0.707106781 * (float)costarr[n - nx]);
      const float de = (float)(0.707106781 * (float)costarr[n + nx]);
      potarr[n] = pot;
      if (astar) {  // updateCellAstar adds the distance to the start AFTER the store: only the threshold and push tests see it
        const int x = n % nx, y = n / nx;
        const float dist = (float)(hypot((double)(x - start0), (double)(y - start1)) * (float)kCostNeutral);
        pot += dist;
      }
      pb.pushNeighbours(pot < curT, n, nx, pot, l, r, u, d, le, re, ue, de, pushable);
    }
  };
  const int cycles = max(nx * ny / 20, nx + ny);
  int cycle = 0;
  if (astar) {
    const float dist = (float)(hypot((double)(goal0 - start0), (double)(goal1 - start1)) * (float)kCostNeutral);
    curT = dist + curT;
  }
  const int startCell = start1 * nx + start0;
  for (; cycle < cycles; cycle++) {
    if (pb.cur_end == 0 && pb.next_end == 0) break;
    pb.beginBlock();
    for (int i = 0; i < pb.cur_end; i++) updateCell(pb.cur[i]);
    pb.endBlock(curT, priInc);
    if (astar || at_start)  // (NavFn stops at the start cell only when asked to; DijkstraExpansion always stops at its goal)
      if (potarr[startCell] < kPotHigh) break;
  }
  return cycle;
}

__global__ __launch_bounds__(256) void k_navfn_plan(NavfnDev nv, uint32_t first, const int32_t* goals, const int32_t* starts, int astar,
                                                    int at_start) {
  const uint32_t plan = first + blockIdx.x;
  const int goal0 = goals[2 * blockIdx.x], goal1 = goals[2 * blockIdx.x + 1];
  const int start0 = starts[2 * blockIdx.x], start1 = starts[2 * blockIdx.x + 1];
  navfnSetup(nv, plan);
  if (threadIdx.x != 0) return;
  const int cycle = navfnPropagate(nv, plan, goal0, goal1, start0, start1, astar, at_start);
  navfnCalcPath(nv, plan, nv.potarr + (size_t)plan * nv.ns_padded, goal0, goal1, start0, start1, astar ? nv.nx * 4 : nv.nx * nv.ny / 2, cycle);
}

// ------------------------------------------------------------------------------------------------
// The expansion as a device algorithm (navgpu_navfn_plan_wavefront): the same update rule - NavFn::updateCell's
// two-neighbour interpolation (navfn.cpp:466-535), float / double arithmetic as written there - relaxed to its FIXED POINT by
// 32 x 32 tiles instead of walked through three priority buffers on one lane.
//   * A tile in LDS (34 x 34 potentials with its halo, 32 x 32 costs) is swept red / black - the four-neighbour stencil is
//     bipartite, so a half-sweep reads only cells of the other colour: race-free, and the same result whatever the waves'
//     timing - until nothing in it changes; then its interior goes back to HBM and the tiles across every edge whose border
//     row changed are marked for the next round.  One launch per round; a launch's workgroups look their tile's mark up and
//     leave if there is none.
//   * Rounds are Jacobi across tiles: round r reads the array round r - 1 wrote (P[(r - 1) & 1]) and writes P[r & 1]; a tile
//     that changed in round r - 1 and is not marked in round r copies itself across, so both arrays stay complete.  Nothing a
//     round reads is written in that round: results do not depend on how the workgroups are scheduled.
//   * Early stop, the counterpart of `if (atStart) if (potarr[startCell] < POT_HIGH) break` (:692-694): an update writes a
//     value above every value it was computed from, so once a round's smallest new value is >= the start cell's potential
//     no later round can write below it - the start cell and everything below its potential are final.  Each round
//     records its number of changed tiles and its smallest new value; the next one reads them before anything else.
// The array this leaves is the update rule's fixed point wherever the potential is below the start cell's, which the
// reference only approaches (its buffers drop entries beyond 10 000, its push tests skip some updates, its early stop leaves
// the last block half done): potentials here are <= the reference's, and the path differs from the reference's by a
// fraction of a cell (tests/test_navfn.py).  The reference-order mode stays the bit-exact one.
// ------------------------------------------------------------------------------------------------
constexpr int kWfTile = 32, kWfThreads = 256;
constexpr uint32_t kWfCopy = 1u, kWfCompute = 2u;

// hf of a cell under a rule: its cost as the update sees it, < 0 = never updated.  navfn: costarr itself, obstacles from COST_OBS
// (navfn.cpp:483); global_planner: DijkstraExpansion::getCost (dijkstra.h:78-87) narrowed to unsigned char as updateCell passes it
// (dijkstra.cpp:178-185)
__device__ __forceinline__ float wfCellCost(const NavfnWfRule& rule, uint8_t cost) {
  if (!rule.global_planner) return cost < kCostObs ? (float)cost : -1.0f;
  float c;
  return gpTraversableCost(cost, rule.lethal_cost, rule.neutral_cost, rule.cost_factor, rule.allow_unknown != 0, c) ? (float)(uint8_t)c : -1.0f;
}

// the arrays a search starts from: POT_HIGH everywhere but the seeds (navfn: the goal, 0 - setupNavFn + initCost :379-453;
// global_planner: the start cell, or setPreciseStart's four cells - dijkstra.cpp:88-110), zero gradients, the outline; the
// tiles that hold a seed or one of its four neighbours are marked for round 0
__global__ __launch_bounds__(256) void k_navfn_wf_init(NavfnDev nv, uint32_t first, NavfnWfRule rule, const int32_t* seed_cells, const float* seed_vals) {
  const uint32_t plan = first + blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= nv.ns) return;
  const int nx = nv.nx, ny = nv.ny;
  const size_t base = (size_t)plan * nv.ns_padded;
  float p0 = kPotHigh;
  bool mark = false;
  for (int k = 0; k < 4; ++k) {
    const int c = seed_cells[4 * blockIdx.y + k];
    if (c < 0) continue;
    if (n == c) p0 = seed_vals[4 * blockIdx.y + k];
    mark = mark || n == c || n == c - 1 || n == c + 1 || n == c - nx || n == c + nx;
  }
  nv.potarr[base + n] = p0;
  nv.potalt[base + n] = p0;
  nv.gradx[base + n] = 0.0f;
  nv.grady[base + n] = 0.0f;
  const int y = n / nx, x = n - y * nx;
  if (rule.outline && (y == 0 || y == ny - 1 || x == 0 || x == nx - 1)) nv.costarr[base + n] = (uint8_t)kCostObs;  // outer bounds of the cost array (254 = LETHAL_OBSTACLE too)
  if (mark) {
    const int tiles = nv.wf_tiles_x * nv.wf_tiles_y;
    atomicOr(&nv.wf_act[((size_t)plan * 2 + 0) * tiles + (y / kWfTile) * nv.wf_tiles_x + x / kWfTile], kWfCompute);
  }
}

__global__ __launch_bounds__(kWfThreads) void k_navfn_wf_round(NavfnDev nv, uint32_t first, NavfnWfRule rule, const int32_t* stop_cells, int at_start, int round) {
  __shared__ float sP[kWfTile + 2][kWfTile + 4];
  __shared__ float sH[kWfTile][kWfTile];
  __shared__ uint32_t s_sides, s_min, s_chg[2];
  const uint32_t plan = first + blockIdx.y;
  const int nx = nv.nx, ny = nv.ny;
  const int tiles = nv.wf_tiles_x * nv.wf_tiles_y;
  const int tile = blockIdx.x, ty = tile / nv.wf_tiles_x, tx = tile - ty * nv.wf_tiles_x;
  const int tid = threadIdx.x;
  NavfnWfStatus* st = nv.wf_status + plan;
  if (st->done) return;
  const size_t base = (size_t)plan * nv.ns_padded;
  const float* Pin = ((round & 1) ? nv.potarr : nv.potalt) + base;  // what round - 1 wrote
  float* Pout = ((round & 1) ? nv.potalt : nv.potarr) + base;
  uint32_t* nchg = nv.wf_nchg + (size_t)plan * nv.wf_max_rounds;
  uint32_t* minv = nv.wf_min + (size_t)plan * nv.wf_max_rounds;
  if (round > 0) {
    const uint32_t changed_tiles = nchg[round - 1];
    const float low = __uint_as_float(minv[round - 1]);  // (0xFFFFFFFF = a NaN when nothing changed: not read then)
    const float ps = Pin[stop_cells[blockIdx.y]];
    if (changed_tiles == 0 || (at_start && ps < kPotHigh && low >= ps)) {
      if (tile == 0 && tid == 0) {
        st->final_array = (round & 1) ^ 1;  // 0: potarr, 1: potalt
        st->rounds = round;
        st->done = 1;
      }
      return;
    }
  }
  uint32_t* act_cur = nv.wf_act + ((size_t)plan * 2 + (round & 1)) * tiles;
  uint32_t* act_nxt = nv.wf_act + ((size_t)plan * 2 + ((round & 1) ^ 1)) * tiles;
  const uint32_t a = act_cur[tile];
  if (a == 0) return;
  if (tid == 0) {
    s_sides = 0;
    s_min = 0xFFFFFFFFu;
    s_chg[0] = s_chg[1] = 0u;
  }
  const int x0 = tx * kWfTile, y0 = ty * kWfTile;
  // ---- load: interior (4 cells per thread, rows of 32 floats), then the halo ring; off the map = an unreached obstacle
  const uint8_t* cost = nv.costarr + base;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + kWfThreads * k, row = i >> 5, col = i & 31;
    const int gx = x0 + col, gy = y0 + row;
    const bool in = gx < nx && gy < ny;
    sP[row + 1][col + 1] = in ? Pin[gy * nx + gx] : kPotHigh;
    const uint8_t c = in ? cost[gy * nx + gx] : (uint8_t)kCostObs;
    // < 0 = not updated ("don't propagate into obstacles", :483).  global_planner: rows 0 and ny - 1 are never updated either - the
    // reference's updateCell would read potential[n - nx] / [n + nx] outside its arrays there (its outlineMap makes those rows lethal by
    // default; with outline_map off the checker, GlobalPlannerOracle::dijkstraFixedPoint, leaves them out the same way)
    sH[row][col] = (rule.global_planner && (gy == 0 || gy == ny - 1)) ? -1.0f : wfCellCost(rule, c);
  }
  if (tid < 128) {
    const int side = tid >> 5, j = tid & 31;  // 0: row above, 1: row below, 2: column left, 3: column right
    const int gx = side == 0 || side == 1 ? x0 + j : (side == 2 ? x0 - 1 : x0 + kWfTile);
    const int gy = side == 0 ? y0 - 1 : (side == 1 ? y0 + kWfTile : y0 + j);
    const bool in = gx >= 0 && gy >= 0 && gx < nx && gy < ny;
    const float v = in ? Pin[gy * nx + gx] : kPotHigh;
    if (side == 0) sP[0][j + 1] = v;
    else if (side == 1) sP[kWfTile + 1][j + 1] = v;
    else if (side == 2) sP[j + 1][0] = v;
    else sP[j + 1][kWfTile + 1] = v;
  }
  __syncthreads();
  bool any_change = false, capped = false;
  if (a & kWfCompute) {
    uint32_t sides = 0;
    float low = kPotHigh * 4.0f;
    int sweeps = 0;
    // a lane's four cells (two per colour): their costs, and the two neighbour minima their last update was computed from - the
    // update is a function of those and the cost alone, so a cell whose minima have not moved is skipped (most cells, most
    // sweeps: the front inside a tile is a cell or two wide)
    float hf4[4], seen_h[4], seen_v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = tid + kWfThreads * (q & 1), row = i >> 4, col = 2 * (i & 15) + ((row + (q >> 1)) & 1);
      hf4[q] = sH[row][col];
      seen_h[q] = seen_v[q] = -1.0f;  // (no potential is negative)
    }
    // "did anything change this sweep" through two alternating LDS flags (any lane that lowers a cell sets this sweep's flag; the
    // other flag is cleared between the two barriers of the sweep, when nobody reads or sets it): two barriers per sweep, where
    // __syncthreads_or costs three of its own
    for (;;) {
      int changed = 0;
      volatile uint32_t* flag = &s_chg[sweeps & 1];
#pragma unroll
      for (int colour = 0; colour < 2; ++colour) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int i = tid + kWfThreads * k, row = i >> 4, col = 2 * (i & 15) + ((row + colour) & 1);
          const int q = 2 * colour + k;
          const float hf = hf4[q];
          const float l = sP[row + 1][col], r = sP[row + 1][col + 2], u = sP[row][col + 1], d = sP[row + 2][col + 1];
          const float tc = l < r ? l : r, ta = u < d ? u : d;
          if (tc == seen_h[q] && ta == seen_v[q]) continue;  // (a cell whose two minima have not moved: the rules below give what they gave)
          seen_h[q] = tc;
          seen_v[q] = ta;
          // PotentialCalculator::calculatePotential (potential_calculator.h:50-59), or the interpolation; hf >= 0 is tested after
          const float pot = !rule.quadratic ? fminf(fminf(l, r), fminf(u, d)) + hf : interpolatePotential(tc, ta, hf);
          if (hf >= 0.0f && pot < sP[row + 1][col + 1]) {
            sP[row + 1][col + 1] = pot;
            changed = 1;
            low = fminf(low, pot);
            sides |= (row == 0 ? 1u : 0u) | (row == kWfTile - 1 ? 2u : 0u) | (col == 0 ? 4u : 0u) | (col == kWfTile - 1 ? 8u : 0u);
          }
        }
        if (colour == 0) {
          if (changed) *flag = 1u;
          changed = 0;
          __syncthreads();
          if (tid == 0) s_chg[(sweeps + 1) & 1] = 0u;
        }
      }
      if (changed) *flag = 1u;
      __syncthreads();
      const uint32_t any = *flag;
      if (!any) break;
      any_change = true;
      if (++sweeps >= rule.max_sweeps) {  // go on next round, with the neighbours' news
        capped = true;
        break;
      }
    }
    if (any_change) {
      // (positive floats order like their bit patterns)
      for (int off = 32; off > 0; off >>= 1) {
        low = fminf(low, __shfl_down(low, off));
        sides |= __shfl_down(sides, off);
      }
      if ((tid & 63) == 0) {
        atomicMin(&s_min, __float_as_uint(low));
        atomicOr(&s_sides, sides);
      }
      __syncthreads();
    }
  }
  if (any_change || (a & kWfCopy)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = tid + kWfThreads * k, row = i >> 5, col = i & 31;
      const int gx = x0 + col, gy = y0 + row;
      if (gx < nx && gy < ny) Pout[gy * nx + gx] = sP[row + 1][col + 1];
    }
  }
  if (tid == 0) {
    act_cur[tile] = 0;  // (read again two rounds on; set only by round + 1)
    if (any_change) {
      const uint32_t sd = s_sides;
      atomicOr(&act_nxt[tile], kWfCopy | (capped ? kWfCompute : 0u));
      if ((sd & 1u) && ty > 0) atomicOr(&act_nxt[tile - nv.wf_tiles_x], kWfCompute);
      if ((sd & 2u) && ty + 1 < nv.wf_tiles_y) atomicOr(&act_nxt[tile + nv.wf_tiles_x], kWfCompute);
      if ((sd & 4u) && tx > 0) atomicOr(&act_nxt[tile - 1], kWfCompute);
      if ((sd & 8u) && tx + 1 < nv.wf_tiles_x) atomicOr(&act_nxt[tile + 1], kWfCompute);
      atomicAdd(&nchg[round], 1u);
      atomicMin(&minv[round], s_min);
    }
  }
}

// NavFn::calcPath / gradCell (:811-1056) by one WAVE: the walk itself is sequential (a step needs the cell and offset the step
// before it left), but a step alone on one lane costs ~3 us of dependent L2 round trips (the 3 x 3 neighbourhood, then four
// gradCell calls of five reads each, memoised through two more arrays).  Here a 64 x 64 window of the potential array around
// the walker sits in LDS (reloaded when the walker comes within two cells of its rim; addressed by FLAT index, so a read that
// runs off a row's end sees what the reference's flat array holds there), the nine neighbourhood reads are nine lanes and a
// ballot, the four gradCell calls four lanes, and every lane carries the walker's state.  gradCell is a pure function of the
// potential array (its gradx / grady memo only saves recomputation), so the arithmetic per value is that of navfnCalcPath,
// expression for expression.
constexpr int kPathWin = 64;
__global__ __launch_bounds__(64) void k_navfn_wf_path(NavfnDev nv, uint32_t first, const int32_t* goals, const int32_t* starts) {
  __shared__ float sW[kPathWin * kPathWin];
  const uint32_t plan = first + blockIdx.x;
  const int lane = threadIdx.x;
  const NavfnWfStatus st = nv.wf_status[plan];
  const float* potarr = (st.final_array ? nv.potalt : nv.potarr) + (size_t)plan * nv.ns_padded;
  const int nx = nv.nx, ny = nv.ny, ns = nv.ns;
  float* pathx = nv.path + (size_t)plan * 2 * nv.path_cap;
  float* pathy = pathx + nv.path_cap;
  const int goal0 = goals[2 * blockIdx.x], goal1 = goals[2 * blockIdx.x + 1];
  const int startCell = starts[2 * blockIdx.x + 1] * nx + starts[2 * blockIdx.x];
  const int n_max = nx * ny / 2;
  const float pot_nx1 = potarr[nx + 1];  // gradCell's `potarr[nx + 1]` (:1020, as written in the reference)
  int wx0 = 0, wy0 = 0;
  bool have_win = false;
  int stc = startCell, npath = 0, found = 0;
  float dx = 0, dy = 0;
  float px1 = 0, py1 = 0, px2 = 0, py2 = 0;  // the two points before the last one (oscillation test)
  for (int i = 0; i < n_max && i < (int)nv.path_cap; i++) {
    const int sy = stc / nx, sx = stc - sy * nx;
    if (!have_win || sx - wx0 < 2 || sx - wx0 > kPathWin - 4 || sy - wy0 < 2 || sy - wy0 > kPathWin - 4) {
      __syncthreads();
      wx0 = sx - kPathWin / 2;
      wy0 = sy - kPathWin / 2;
      for (int k = lane; k < kPathWin * kPathWin; k += 64) {
        const int j = k / kPathWin, c = k - j * kPathWin;
        const long n = (long)(wy0 + j) * nx + (wx0 + c);
        sW[k] = (n >= 0 && n < ns) ? potarr[n] : kPotHigh;
      }
      have_win = true;
      __syncthreads();
    }
    auto P = [&](int ox, int oy) -> float { return sW[(sy - wy0 + oy) * kPathWin + (sx - wx0 + ox)]; };  // potarr[stc + ox + oy * nx]
    {
      const int want = stc + (int)round((double)dx) + (int)(nx * round((double)dy));
      const int nearest_point = max(0, min(nx * ny - 1, want));
      const float pn = nearest_point == want ? P((int)round((double)dx), (int)round((double)dy)) : potarr[nearest_point];
      if (pn < (float)kCostNeutral) {
        if (lane == 0) {
          pathx[npath] = (float)goal0;
          pathy[npath] = (float)goal1;
        }
        ++npath;
        found = 1;
        break;
      }
    }
    if (stc < nx || stc > ns - nx) break;  // would be out of bounds
    const float cx = (float)(stc % nx) + dx, cy = (float)(stc / nx) + dy;
    if (lane == 0) {
      pathx[npath] = cx;
      pathy[npath] = cy;
    }
    npath++;
    const bool oscillation_detected = npath > 2 && cx == px2 && cy == py2;
    px2 = px1;
    py2 = py1;
    px1 = cx;
    py1 = cy;
    const int l9 = lane < 9 ? lane : 0;
    const bool high9 = lane < 9 && P(l9 % 3 - 1, l9 / 3 - 1) >= kPotHigh;
    if (__ballot(high9) != 0ull || oscillation_detected) {
      int mox, moy;
      lowestOfEight(P, mox, moy);
      const float pm = P(mox, moy);
      stc += mox + moy * nx;
      dx = 0;
      dy = 0;
      if (pm >= kPotHigh) break;
    } else {
      // gradCell of stc, stc + 1, stc + nx, stc + nx + 1 on lanes 0..3 (no memo: it only saves recomputation)
      const int q = lane & 3, qx = q & 1, qy = q >> 1;
      float gx, gy;
      cellGradient(P, qx, qy, stc + qx + qy * nx, nx, ns, pot_nx1, (float)kCostObs, gx, gy);
      const float gxs[4] = {__shfl(gx, 0), __shfl(gx, 1), __shfl(gx, 2), __shfl(gx, 3)};
      const float gys[4] = {__shfl(gy, 0), __shfl(gy, 1), __shfl(gy, 2), __shfl(gy, 3)};
      if (!gradientStep(gxs, gys, nx, stc, dx, dy)) break;  // zero gradient
    }
  }
  if (lane == 0) {
    navgpu_navfn_result r;
    r.found = found;
    r.path_length = found ? npath : 0;
    r.cycles = st.rounds;
    r.start_potential = potarr[startCell];
    nv.results[plan] = r;
  }
}

// ------------------------------------------------------------------------------------------------
// global_planner (the other half of SURVEY 8 f-4): what GlobalPlanner::makePlan runs between worldToMap and the plan
// assembly (global_planner/src/planner_core.cpp:250-306) -
//   outlineMap (:62-76), DijkstraExpansion::calculatePotentials / updateCell / getCost (dijkstra.cpp:71-229, dijkstra.h:78-87)
//   or AStarExpansion::calculatePotentials / add (astar.cpp:46-95: std::push_heap / pop_heap with greater1),
//   PotentialCalculator / QuadraticCalculator::calculatePotential (potential_calculator.h:50-59, quadratic_calculator.cpp:41-77),
//   Expander::clearEndpoint (expander.h:76-89), GradientPath::getPath / gradCell (gradient_path.cpp:68-313) or
//   GridPath::getPath (grid_path.cpp:44-82).
// Same kind of process as NavFn's (priority buffers in buffer order, early stop at the goal cell), same treatment: one
// lane per plan, bit for bit.  costarr holds the raw costmap bytes (navgpu_navfn_set_costmap with cost_mode 0).
// ------------------------------------------------------------------------------------------------
struct GpHeapEntry {  // astar.h:47-55 Index
  int i;
  float cost;
};

// One plan as the stages below see it: its arrays, its end points and the cost / potential rules its parameters select.
// A border cell can enter the expansion when nothing outlines the map (outline_map == 0) or when the outline's 254 is
// below lethal_cost (A* with lethal_cost 255).  The reference then reads potential[n - nx] / costs[n + nx] outside its
// arrays (harmless garbage on the CPU heap); here every neighbour access goes through potAt() / getCost(), which give
// an off-array cell the values of an unreached lethal one.  In-array reads are unchanged, bit for bit.
struct GpPlan {
  int nx, ny, ns;
  uint8_t *costs, *pending;
  float *potential, *gradx, *grady;
  double start_x, start_y, goal_x, goal_y;
  int lethal, neutral;
  float factor;
  bool unknown, quadratic;
  __device__ __forceinline__ int startCell() const { return (int)start_x + nx * (int)start_y; }
  __device__ __forceinline__ int endCell() const { return (int)goal_x + nx * (int)goal_y; }
  __device__ __forceinline__ int maxCycles() const { return nx * ny * 2; }
  __device__ __forceinline__ float potAt(int n) const { return (n >= 0 && n < ns) ? potential[n] : kPotHigh; }
  __device__ __forceinline__ float getCost(int n) const {  // DijkstraExpansion::getCost: what is not traversable costs lethal_cost
    float c;
    return (n >= 0 && n < ns && gpTraversableCost(costs[n], lethal, neutral, factor, unknown, c)) ? c : (float)lethal;
  }
  // PotentialCalculator / QuadraticCalculator::calculatePotential (potential_calculator.h:50-59, quadratic_calculator.cpp:41-77)
  __device__ __forceinline__ float calculatePotential(uint8_t cost, int n, float prev_potential) const {
    if (!quadratic && !(prev_potential < 0)) return prev_potential + cost;
    const float l = potAt(n - 1), r = potAt(n + 1), u = potAt(n - nx), d = potAt(n + nx);
    if (quadratic) return interpolatePotential(l < r ? l : r, u < d ? u : d, cost);
    return fminf(fminf(l, r), fminf(u, d)) + cost;
  }
};
__device__ __forceinline__ GpPlan gpPlanOf(const NavfnDev& nv, uint32_t plan, const navgpu_global_planner_params& gp, const double* starts,
                                           const double* goals, float* potential) {
  const size_t base = (size_t)plan * nv.ns_padded;
  GpPlan p;
  p.nx = nv.nx, p.ny = nv.ny, p.ns = nv.ns;
  p.costs = nv.costarr + base, p.pending = nv.pending + base;
  p.potential = potential, p.gradx = nv.gradx + base, p.grady = nv.grady + base;
  p.start_x = starts[2 * blockIdx.x], p.start_y = starts[2 * blockIdx.x + 1];
  p.goal_x = goals[2 * blockIdx.x], p.goal_y = goals[2 * blockIdx.x + 1];
  p.lethal = gp.lethal_cost, p.neutral = gp.neutral_cost, p.factor = gp.cost_factor;
  p.unknown = gp.allow_unknown != 0, p.quadratic = gp.use_quadratic != 0;
  return p;
}

// all lanes: the arrays every expansion starts from, and GlobalPlanner::outlineMap (planner_core.cpp:62-76)
__device__ __forceinline__ void gpSetup(const GpPlan& p, bool outline_map) {
  for (int i = threadIdx.x; i < p.ns; i += blockDim.x) {
    p.potential[i] = kPotHigh;
    p.gradx[i] = 0.0f;
    p.grady[i] = 0.0f;
    p.pending[i] = 0;
    const int y = i / p.nx, x = i - y * p.nx;
    if (outline_map && (y == 0 || y == p.ny - 1 || x == 0 || x == p.nx - 1)) p.costs[i] = 254;  // costmap_2d::LETHAL_OBSTACLE
  }
  __syncthreads();
}

// DijkstraExpansion::calculatePotentials / updateCell (dijkstra.cpp:71-229), one lane: whether a legal potential was found
__device__ bool gpDijkstra(const GpPlan& p, int* buffers, bool precise_start, int& cycle) {
  const int nx = p.nx, lethal = p.lethal;
  float* potential = p.potential;
  PriorityBuffers pb(buffers, p.pending, p.ns);
  float threshold = lethal;
  // The constructor's 2 * 50 (dijkstra.cpp:49), whatever neutral_cost is configured: GlobalPlanner sets the cost through its
  // Expander* member (planner_core.cpp:170), Expander::setNeutralCost is not virtual (expander.h:67), and so
  // DijkstraExpansion::setNeutralCost, which would recompute the increment, is never the one called.
  const float priorityIncrement = 2 * 50;
  auto pushable = [&](int n) { return p.getCost(n) < lethal; };
  const int k = p.startCell();
  if (precise_start) {  // setPreciseStart(true) (planner_core.cpp:124-127)
    int cells[4];
    float vals[4];
    preciseStartSeeds(p.start_x, p.start_y, nx, p.neutral, cells, vals);
    const int around[8] = {k + 2, k - 1, k + nx - 1, k + nx + 2, k - nx, k - nx + 1, k + nx * 2, k + nx * 2 + 1};
#pragma unroll
    for (int i = 0; i < 4; ++i) potential[cells[i]] = vals[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) pb.pushCur(around[i], pushable);
  } else {
    potential[k] = 0;
    pb.pushCur(k + 1, pushable);
    pb.pushCur(k - 1, pushable);
    pb.pushCur(k - nx, pushable);
    pb.pushCur(k + nx, pushable);
  }
  const int cycles = p.maxCycles(), endCell = p.endCell();
  bool ran_dry = false;
  for (; cycle < cycles; cycle++) {
    if (pb.cur_end == 0 && pb.next_end == 0) {
      ran_dry = true;
      break;
    }
    pb.beginBlock();
    for (int i = 0; i < pb.cur_end; i++) {  // updateCell
      const int n = pb.cur[i];
      const float c = p.getCost(n);
      if (c >= lethal) continue;
      const float pot = p.calculatePotential((uint8_t)c, n, -1.0f);
      if (pot < potential[n]) {
        const float le = (float)(0.707106781 * (float)p.getCost(n - 1));
        const float re = (float)(0.707106781 * (float)p.getCost(n + 1));
        const float ue = (float)(0.707106781 * (float)p.getCost(n - nx));
        const float de = (float)(0.707106781 * (float)p.getCost(n + nx));
        potential[n] = pot;
        pb.pushNeighbours(pot < threshold, n, nx, pot, p.potAt(n - 1), p.potAt(n + 1), p.potAt(n - nx), p.potAt(n + nx), le, re, ue, de, pushable);
      }
    }
    pb.endBlock(threshold, priorityIncrement);
    if (potential[endCell] < kPotHigh) break;  // (always, where NavFn stops only when asked to; a dry run is told apart above)
  }
  return !ran_dry && cycle < cycles;
}

// AStarExpansion::calculatePotentials / add (astar.cpp:46-95: std::push_heap / pop_heap with greater1), one lane
__device__ bool gpAstar(const GpPlan& p, GpHeapEntry* heap, int& cycle) {
  const int nx = p.nx, ns = p.ns, lethal = p.lethal, neutral = p.neutral;
  float* potential = p.potential;
  const uint8_t* costs = p.costs;
  long len = 0;
  auto pushHeap = [&](long hole, const GpHeapEntry value) {  // std::__push_heap with greater1: parent.cost > value.cost moves down
    long parent = (hole - 1) / 2;
    while (hole > 0 && heap[parent].cost > value.cost) {
      heap[hole] = heap[parent];
      hole = parent;
      parent = (hole - 1) / 2;
    }
    heap[hole] = value;
  };
  const int start_i = p.startCell(), endCell = p.endCell(), cycles = p.maxCycles();
  heap[len++] = GpHeapEntry{start_i, 0.0f};  // queue_.push_back(Index(start_i, 0)) - no push_heap on the first element
  potential[start_i] = 0;
  const int ex = (int)p.goal_x, ey = (int)p.goal_y;
  auto add = [&](float prev_potential, int next_i) {
    if (next_i < 0 || next_i >= ns) return;
    if (potential[next_i] < kPotHigh) return;
    if (costs[next_i] >= lethal && !(p.unknown && costs[next_i] == 255)) return;
    potential[next_i] = p.calculatePotential((uint8_t)(costs[next_i] + neutral), next_i, prev_potential);
    const int x = next_i % nx, y = next_i / nx;
    const float distance = (float)(abs(ex - x) + abs(ey - y));
    pushHeap(len, GpHeapEntry{next_i, potential[next_i] + distance * neutral});
    ++len;
  };
  while (len > 0 && cycle < cycles) {
    const GpHeapEntry top = heap[0];
    if (len > 1) {  // std::pop_heap: __adjust_heap(first, 0, len - 1, value = last element)
      const GpHeapEntry value = heap[len - 1];
      const long l = len - 1;
      long hole = 0, child = 0;
      while (child < (l - 1) / 2) {
        child = 2 * (child + 1);
        if (heap[child].cost > heap[child - 1].cost) child--;
        heap[hole] = heap[child];
        hole = child;
      }
      if ((l & 1) == 0 && child == (l - 2) / 2) {
        child = 2 * (child + 1);
        heap[hole] = heap[child - 1];
        hole = child - 1;
      }
      pushHeap(hole, value);
    }
    --len;
    const int i = top.i;
    if (i == endCell) return true;
    add(potential[i], i + 1);
    add(potential[i], i - 1);
    add(potential[i], i + nx);
    add(potential[i], i - nx);
    cycle++;
  }
  return false;
}

// Expander::clearEndpoint(costs, potential, goal_x_i, goal_y_i, 2) (expander.h:76-89)
__device__ void gpClearEndpoint(const GpPlan& p, int goal_cell) {
  for (int i = -2; i <= 2; i++)
    for (int j = -2; j <= 2; j++) {
      const int n = goal_cell + i + p.nx * j;
      if (n < p.nx + 1 || n >= p.ns - p.nx - 1) continue;  // (the reference reads outside its arrays for a goal this close to the border)
      if (p.potential[n] < kPotHigh) continue;
      // `float c = costs[n] + neutral_cost_` handed to an unsigned char parameter (expander.h:84-85) is out of range from 256 on;
      // amd64 converts through a 32-bit integer and keeps the low byte - the sum (0 ... 510, exact in a float) modulo 256.
      // Stated in integers: what a float-to-byte conversion of such a value gives is not defined on this target either.
      p.potential[n] = p.calculatePotential((uint8_t)((p.costs[n] + p.neutral) & 0xff), n, -1.0f);
    }
}

// the traceback's points: every one counted, those that fit the buffer stored, the last three kept (all of it may not fit)
struct GpPathOut {
  float *x, *y;
  int cap, n = 0;
  float last3x[3] = {0, 0, 0}, last3y[3] = {0, 0, 0};
  __device__ __forceinline__ void push(float px, float py) {
    if (n < cap) {
      x[n] = px;
      y[n] = py;
    }
    last3x[0] = last3x[1];
    last3y[0] = last3y[1];
    last3x[1] = last3x[2];
    last3y[1] = last3y[2];
    last3x[2] = px;
    last3y[2] = py;
    ++n;
  }
};

// GradientPath::getPath / gradCell (gradient_path.cpp:68-313), one lane, from the goal down to the start: 1 = arrived
__device__ int gpGradientPath(const GpPlan& p, GpPathOut& out) {
  const int nx = p.nx, ns = p.ns;
  const float *potential = p.potential;
  float *gradx = p.gradx, *grady = p.grady;
  const float pot_nx1 = potential[nx + 1];
  int stc = p.endCell();
  float dx = (float)(p.goal_x - (int)p.goal_x), dy = (float)(p.goal_y - (int)p.goal_y);
  auto pot = [&](int ox, int oy) -> float { return p.potAt(stc + ox + oy * nx); };
  auto gradCell = [&](int qx, int qy) {  // GradientPath tests the memo second (its gradx_[n] read may lie past the array; never here)
    const int n = stc + qx + qy * nx;
    if (n < nx || n > ns - nx) return;
    if (gradx[n] + grady[n] > 0.0) return;
    float gx, gy;
    if (cellGradient(pot, qx, qy, n, nx, ns, pot_nx1, (float)p.lethal, gx, gy)) {
      gradx[n] = gx;
      grady[n] = gy;
    }
  };
  auto gAt = [&](const float* g, int n) -> float { return n < ns ? g[n] : 0.0f; };  // (stc on the last row: the reference reads past its arrays)
  const long lim = (long)ns * 4;
  long c = 0;
  while (c++ < lim) {
    const double px = stc % nx + dx, py = stc / nx + dy;
    if (fabs(px - p.start_x) < .5 && fabs(py - p.start_y) < .5) {  // (in double, against the start itself, where NavFn looks at a potential)
      out.push((float)p.start_x, (float)p.start_y);
      return 1;
    }
    if (stc < nx || stc > ns - nx) break;
    out.push((float)px, (float)py);
    const bool oscillation_detected = out.n > 2 && out.last3x[2] == out.last3x[0] && out.last3y[2] == out.last3y[0];
    if (highAmongNine(pot) || oscillation_detected) {
      int mox, moy;
      lowestOfEight(pot, mox, moy);
      stc += mox + moy * nx;
      dx = 0;
      dy = 0;
      if (potential[stc] >= kPotHigh) break;
    } else {
      gradCell(0, 0);
      gradCell(1, 0);
      gradCell(0, 1);
      gradCell(1, 1);
      const int stcnx = stc + nx;
      const float gx[4] = {gradx[stc], gAt(gradx, stc + 1), gAt(gradx, stcnx), gAt(gradx, stcnx + 1)};
      const float gy[4] = {grady[stc], gAt(grady, stc + 1), gAt(grady, stcnx), gAt(grady, stcnx + 1)};
      if (!gradientStep(gx, gy, nx, stc, dx, dy)) break;
    }
  }
  return 0;
}

// GridPath::getPath (grid_path.cpp:44-82), one lane: 1 = arrived
__device__ int gpGridPath(const GpPlan& p, GpPathOut& out) {
  const int nx = p.nx, ns = p.ns;
  float cx = (float)p.goal_x, cy = (float)p.goal_y;
  const int start_index = p.startCell();
  out.push(cx, cy);
  long c = 0;
  while ((int)cx + nx * (int)cy != start_index) {
    float min_val = 1e10f;
    int min_x = 0, min_y = 0;
    for (int xd = -1; xd <= 1; xd++)
      for (int yd = -1; yd <= 1; yd++) {
        if (xd == 0 && yd == 0) continue;
        const int x = (int)(cx + xd), y = (int)(cy + yd);
        const int index = x + nx * y;
        if (index < 0 || index >= ns) continue;  // (the reference reads outside its array here)
        if (p.potential[index] < min_val) {
          min_val = p.potential[index];
          min_x = x;
          min_y = y;
        }
      }
    if (min_x == 0 && min_y == 0) return 0;
    cx = (float)min_x;
    cy = (float)min_y;
    out.push(cx, cy);
    if (c++ > (long)ns * 4) return 0;
  }
  return 1;
}

// makePlan's tail (planner_core.cpp:299-311), one lane: clearEndpoint, the traceback - only when a legal potential was found -
// and the result record
__device__ void gpFinish(const NavfnDev& nv, uint32_t plan, const GpPlan& p, const navgpu_global_planner_params& gp, const int32_t* goal_cells,
                         bool found_legal, int cycle) {
  if (!gp.old_navfn_behavior) gpClearEndpoint(p, goal_cells[2 * blockIdx.x] + p.nx * goal_cells[2 * blockIdx.x + 1]);
  GpPathOut out;
  out.x = nv.path + (size_t)plan * 2 * nv.path_cap;
  out.y = out.x + nv.path_cap;
  out.cap = (int)nv.path_cap;
  int found = 0;
  if (found_legal) found = gp.use_grid_path ? gpGridPath(p, out) : gpGradientPath(p, out);
  navgpu_navfn_result r;
  r.found = (found && out.n <= out.cap) ? 1 : 0;
  r.path_length = r.found ? out.n : 0;
  r.cycles = cycle;
  r.start_potential = p.potential[p.endCell()];
  nv.results[plan] = r;
}

__global__ __launch_bounds__(256) void k_gp_plan(NavfnDev nv, uint32_t first, navgpu_global_planner_params gp, const double* starts, const double* goals,
                                                 const int32_t* goal_cells, GpHeapEntry* heaps) {
  const uint32_t plan = first + blockIdx.x;
  const GpPlan p = gpPlanOf(nv, plan, gp, starts, goals, nv.potarr + (size_t)plan * nv.ns_padded);
  gpSetup(p, gp.outline_map != 0);
  if (threadIdx.x != 0) return;
  int cycle = 0;
  const bool found_legal = gp.use_dijkstra ? gpDijkstra(p, nv.pb + (size_t)plan * 3 * kPriorityBufSize, !gp.old_navfn_behavior, cycle)
                                           : gpAstar(p, heaps + (size_t)plan * nv.ns_padded, cycle);
  gpFinish(nv, plan, p, gp, goal_cells, found_legal, cycle);
}
// The expansion has already run as a tiled wavefront (k_navfn_wf_round with the global_planner rule): what remains is makePlan's
// tail on one lane, the stages the reference-order kernel ends with.  The reference leaves its loop through `break` exactly when
// the goal cell has a potential.
__global__ __launch_bounds__(64) void k_gp_wf_finish(NavfnDev nv, uint32_t first, navgpu_global_planner_params gp, const double* starts, const double* goals,
                                                     const int32_t* goal_cells) {
  const uint32_t plan = first + blockIdx.x;
  if (threadIdx.x != 0) return;
  const NavfnWfStatus st = nv.wf_status[plan];
  const GpPlan p = gpPlanOf(nv, plan, gp, starts, goals, (st.final_array ? nv.potalt : nv.potarr) + (size_t)plan * nv.ns_padded);
  gpFinish(nv, plan, p, gp, goal_cells, p.potential[p.endCell()] < kPotHigh, st.rounds);
}

void launch_navfn_costmap(const NavfnDev& nv, uint32_t first, uint32_t count, const uint8_t* cmap, size_t stride, int cost_mode, int allow_unknown,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_navfn_costmap, dim3((nv.ns + 255) / 256, count), dim3(256), 0, s, nv, first, cmap, stride, cost_mode, allow_unknown);
}
void launch_navfn_plan(const NavfnDev& nv, uint32_t first, uint32_t count, const int32_t* goals, const int32_t* starts, int astar, int at_start,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_navfn_plan, dim3(count), dim3(256), 0, s, nv, first, goals, starts, astar, at_start);
}

void launch_navfn_wf_init(const NavfnDev& nv, uint32_t first, uint32_t count, const NavfnWfRule& rule, const int32_t* seed_cells, const float* seed_vals,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_navfn_wf_init, dim3((nv.ns + 255) / 256, count), dim3(256), 0, s, nv, first, rule, seed_cells, seed_vals);
}
void launch_navfn_wf_round(const NavfnDev& nv, uint32_t first, uint32_t count, const NavfnWfRule& rule, const int32_t* stop_cells, int at_start, int round,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_navfn_wf_round, dim3(nv.wf_tiles_x * nv.wf_tiles_y, count), dim3(kWfThreads), 0, s, nv, first, rule, stop_cells, at_start, round);
}
void launch_gp_wf_finish(const NavfnDev& nv, uint32_t first, uint32_t count, const navgpu_global_planner_params& gp, const double* starts,
                         const double* goals, const int32_t* goal_cells, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_wf_finish, dim3(count), dim3(64), 0, s, nv, first, gp, starts, goals, goal_cells);
}
void launch_navfn_wf_path(const NavfnDev& nv, uint32_t first, uint32_t count, const int32_t* goals, const int32_t* starts, hipStream_t s) {
  hipLaunchKernelGGL(k_navfn_wf_path, dim3(count), dim3(64), 0, s, nv, first, goals, starts);
}

void launch_gp_plan(const NavfnDev& nv, uint32_t first, uint32_t count, const navgpu_global_planner_params& gp, const double* starts,
                    const double* goals, const int32_t* goal_cells, void* heaps, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_plan, dim3(count), dim3(256), 0, s, nv, first, gp, starts, goals, goal_cells, static_cast<GpHeapEntry*>(heaps));
}

}  // namespace navgpu
