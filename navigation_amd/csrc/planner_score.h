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
constexpr uint32_t kSweepAuxMinRot = 10;  // aux[10..11]: the robot's min_rot_vel as a double (aux[0..8]: storeSweepRobotScalars, storeFreeDistance)
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
size_t score_prep_free_lds_bytes(const PlannerDev& pl);  // dynamic LDS of a workgroup that runs scorePrepFree (pl.tab_bytes set)
void score_prep_tab_sizes(PlannerDev& pl);               // sets pl.tab_bytes and pl.prep_bytes for the sweep's image
uint32_t launch_score_sweep(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s);  // returns blocks per instance
uint32_t launch_score_sweep_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s);  // the same for a robot list


// ---- the stages that build a robot's image (k_score_prep_*, scoreExplicit, checkTraj, and the prep workgroups of k_bfs_rows)
// The robot a workgroup works on (blockIdx.y) and its costmap window in LDS: win x win cells from map cell (wx0, wy0)
struct ScoreRobot {
  uint32_t inst;
  Geom g;
  navgpu_robot_state st;
  const uint8_t* master;
  const uint32_t *dpath, *dgoal, *dfront;
  const int32_t* cnt;
  uint32_t nfp;
  int win, wx0, wy0;
  int win_bytes, nw;  // the window's bytes rounded up to 16, 32-cell words per window row
};
__device__ __forceinline__ ScoreRobot scoreRobot(const PlannerDev& pl, uint32_t inst) {
  ScoreRobot r;
  r.inst = inst;
  r.g = geomOf(pl, inst);
  r.st = pl.state[inst];
  r.master = pl.master + (size_t)inst * pl.cells_padded;
  r.dpath = pl.path + (size_t)inst * pl.cells;
  r.dgoal = pl.goal + (size_t)inst * pl.cells;
  r.dfront = pl.goal_front + (size_t)inst * pl.cells;
  r.cnt = pl.axis_count + 4 * inst;
  r.nfp = pl.fp_n[inst];
  r.win = (int)pl.win;
  r.win_bytes = (r.win * r.win + 15) & ~15;
  r.nw = (r.win + 31) >> 5;
  return r;
}
// the window's origin: robot cell (floor of the map coordinate, also valid when the robot is off the map) - win / 2
__device__ __forceinline__ void placeWindow(ScoreRobot& r) {
  double fx = floor(((double)r.st.pos[0] - r.g.ox) / r.g.res), fy = floor(((double)r.st.pos[1] - r.g.oy) / r.g.res);
  fx = fmin(fmax(fx, -1.0e6), 1.0e6);
  fy = fmin(fmax(fy, -1.0e6), 1.0e6);
  r.wx0 = (int)fx - r.win / 2;
  r.wy0 = (int)fy - r.win / 2;
}

// ---- stage: footprint and per-axis samples (not for an explicit sample) to LDS, the workgroup's counters cleared, the
// window placed and its bytes staged
template <bool EXPLICIT>
__device__ __forceinline__ void stageInputs(const PlannerDev& pl, ScoreRobot& r, double* s_fp, float (*s_axis)[kMaxAxis], int* s_cnt, uint8_t* s_win) {
  const uint32_t tid = threadIdx.x;
  const Geom& g = r.g;
  if (tid < 2 * r.nfp) s_fp[tid] = pl.fp_spec[(size_t)r.inst * kMaxFootprint * 2 + tid];
  if (!EXPLICIT) {
    for (uint32_t i = tid; i < 3 * kMaxAxis; i += blockDim.x) {
      uint32_t a = i / kMaxAxis, k = i - a * kMaxAxis;
      s_axis[a][k] = k < pl.max_axis ? pl.axis_samples[((size_t)r.inst * 3 + a) * pl.max_axis + k] : 0.f;
    }
  }
  if (tid == 0) s_cnt[0] = s_cnt[1] = 0;
  placeWindow(r);
  const int win = r.win, wx0 = r.wx0, wy0 = r.wy0;
  // (eight loads of a lane in flight at a time - unconditional, clamped: a conditional load in a rolled loop is waited
  // for on its own, nine latencies in a row for a 65 x 65 window)
  for (int i0 = tid; i0 < win * win; i0 += 8 * (int)blockDim.x) {
    uint8_t v[8];
    bool in_map[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ic = min(i0 + u * (int)blockDim.x, win * win - 1);
      const int ly = ic / win, lx = ic - ly * win;
      const int gx = wx0 + lx, gy = wy0 + ly;
      in_map[u] = gx >= 0 && gy >= 0 && gx < (int)g.nx && gy < (int)g.ny;
      v[u] = r.master[min(max(gy, 0), (int)g.ny - 1) * g.nx + min(max(gx, 0), (int)g.nx - 1)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * (int)blockDim.x;
      if (i < win * win) s_win[i] = in_map[u] ? v[u] : (uint8_t)0;
    }
  }
}

// ---- stage: per-cell screens of the window, four bitmaps interleaved per 32-cell word: s_fb[(y * nw + j) * 4 + k]
// Footprint shortcuts: the cells a footprint with centre cell c can touch lie within the Chebyshev radius
// fp_rcells of c (>= circumscribed radius in cells + 1).  Two bitmaps of the window, dilated by that radius, are
// built once per robot (bit-parallel: rows of 32-cell words, shifts for the horizontal pass, word ORs for the
// vertical one; everything outside the window or off the map counts as set):
//   k = 0: some cell in reach is not FREE_SPACE  -> clear = the point's footprint cost is exactly 0
//   k = 1: some cell in reach fails pointCost    -> clear = the point is legal (cost not needed)
// MapGrid screens (not dilated): a trajectory point only has to NOT be an obstacle / unreachable cell of the path and
// goal grids unless it is the last one (aggregation Last, map_grid_cost_function.cpp:92-127):
//   k = 2: path grid holds obstacleCosts() or unreachableCellCosts() here    k = 3: the goal grid does
// s_ba: build scratch behind the image (window + bitmaps + tables): [win][nw][2] raw, [win][nw][2] after the horizontal pass.
// The LDS window is kept in "walk order": with allow_unknown the bytes 254 (LETHAL) and 255 (NO_INFORMATION)
// are swapped, so that in both modes a footprint cell fails pointCost iff its stored byte >= walk_fail and the
// polygon walk needs nothing but a running maximum per cell (cellCost() undoes the swap).
// The stage comes in three parts, so that the part that reads the path and goal grids can run apart from the rest (scorePrepFree /
// k_score_prep_grids): the footprint screens (words 0 and 1; GRIDS false: words 2 and 3 are stored as zero with them), the MapGrid
// screens (words 2 and 3), the walk order.  buildScreens is the three in a row.
template <bool GRIDS>
__device__ __forceinline__ void buildFootprintScreens(const PlannerDev& pl, const ScoreRobot& r, uint8_t* s_dyn, uint32_t* s_ba) {
  const uint32_t tid = threadIdx.x;
  const Geom& g = r.g;
  const int win = r.win, wx0 = r.wx0, wy0 = r.wy0, nw = r.nw;
  const uint8_t* s_win = s_dyn;
  uint32_t* s_fb = reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes);  // [win][nw][4]
  const int rc = (int)pl.fp_rcells;
  const uint8_t fail_span_w = (pl.cfg.allow_unknown != 0) ? 0 : 1;
  {  // the raw bits: 64 consecutive cells of a (padded) window row per wave step, packed by ballot
    const int row_cells = nw * 32;
    const bool obst_off = pl.scale_obstacle == 0;  // obstacle critic off (scale 0: skipped, simple_scored_sampling_planner.cpp:55-57): nothing to screen
    for (int base = (int)(tid & ~63u); base < win * row_cells; base += (int)blockDim.x) {
      const int idx = base + (int)(tid & 63u);
      const int y = idx / row_cells, lx = idx - y * row_cells;
      // cells off the MAP count as set like cells outside the window: a footprint vertex there fails
      // worldToMap, i.e. footprintCost = -1 (costmap_model.cpp:77-99), which only the polygon walk reports
      const int gx = wx0 + lx, gy = wy0 + y;
      const bool in = lx < win && y < win && gx >= 0 && gy >= 0 && gx < (int)g.nx && gy < (int)g.ny;
      const uint8_t cc = s_win[in ? y * win + lx : 0];
      const bool o = !obst_off && (!in || cc != 0), f = !obst_off && (!in || (uint8_t)(cc - kLethal) <= fail_span_w);
      const unsigned long long mo = __ballot(o), mf = __ballot(f);
      if ((tid & 63u) == 0) {
        const int w = idx >> 5;  // linear word index y * nw + j; a wave covers two words (possibly of two rows)
        s_ba[2 * w] = (uint32_t)mo;
        s_ba[2 * w + 1] = (uint32_t)mf;
        if (w + 1 < win * nw) {
          s_ba[2 * (w + 1)] = (uint32_t)(mo >> 32);
          s_ba[2 * (w + 1) + 1] = (uint32_t)(mf >> 32);
        }
      }
    }
  }
  __syncthreads();
  // The dilation: a DISC (PlannerDev::fp_halfw: per row offset dy the largest |dx| an outline cell can have), not the Chebyshev
  // square around it - a fifth to a quarter fewer cells, and every cell less is trajectory points that need not be looked at.
  // Grouped by dx: the rows that contribute at |dx| = d are |dy| <= Y(d) (the half widths fall with |dy|), so the rows are OR-ed
  // in from the centre outwards (the word and its two neighbours) and row offset Y shifts the running OR by the d's it is the
  // last row for: halfw[Y + 1] < d <= halfw[Y].  One shift pair per d instead of one per cell of the disc.
  for (int it = tid; it < 2 * win * nw; it += blockDim.x) {
    const int cell = it >> 1;
    const int y = cell / nw, j = cell - y * nw;
    uint32_t m = (y - rc < 0 || y + rc >= win || rc > 31) ? 0xFFFFFFFFu : 0u;  // (reach beyond the neighbouring words: no shortcut)
    if (!m) {
      uint32_t vc = 0, vl = j > 0 ? 0u : 0xFFFFFFFFu, vr = j + 1 < nw ? 0u : 0xFFFFFFFFu;
      for (int Y = 0; Y <= rc; ++Y) {
        const int w = (int)pl.fp_halfw[Y];
        if (w == 0xFF) break;
        const int up = it + 2 * Y * nw, dn = it - 2 * Y * nw;
        vc |= s_ba[up] | s_ba[dn];
        if (j > 0) vl |= s_ba[up - 2] | s_ba[dn - 2];
        if (j + 1 < nw) vr |= s_ba[up + 2] | s_ba[dn + 2];
        const int wn = (Y + 1 <= rc && pl.fp_halfw[Y + 1] != 0xFF) ? (int)pl.fp_halfw[Y + 1] : -1;  // (the outermost row: every d down to 0)
        for (int d = wn + 1; d <= w; ++d) m |= d == 0 ? vc : (__builtin_amdgcn_alignbit(vc, vl, 32 - d) | __builtin_amdgcn_alignbit(vr, vc, d));
      }
    }
    s_fb[4 * cell + (it & 1)] = m;
    if (!GRIDS) s_fb[4 * cell + 2 + (it & 1)] = 0u;
  }
}
// the path / goal screen bits of the 64 cells of a wave step: cells outside the window or off the map count as set; a critic with
// scale 0 is never evaluated, its screen stays clear
__device__ __forceinline__ void gridScreenBits(const PlannerDev& pl, bool in, uint32_t dp, uint32_t dg, unsigned long long& mp, unsigned long long& mg) {
  const uint32_t n_obst = pl.cells, n_unreach = pl.cells + 1;
  bool pf = true, gf = true;
  if (in) {
    pf = dp == n_obst || dp == n_unreach;
    gf = dg == n_obst || dg == n_unreach;
  }
  pf = pf && pl.scale_path != 0;
  gf = gf && pl.scale_goal != 0;
  mp = __ballot(pf);
  mg = __ballot(gf);
}
// STEPS: steps of a wave whose loads are in flight together (2 * STEPS per lane); s_fb: the screens [win][nw][4]
template <int STEPS>
__device__ __forceinline__ void buildGridScreens(const PlannerDev& pl, const ScoreRobot& r, uint32_t* s_fb) {
  const uint32_t tid = threadIdx.x;
  const Geom& g = r.g;
  const int win = r.win, wx0 = r.wx0, wy0 = r.wy0, nw = r.nw;
  const uint32_t *dpath = r.dpath, *dgoal = r.dgoal;
  {  // MapGrid screens: 64 consecutive cells of a (padded) window row per wave step, packed by ballot
    const int row_cells = nw * 32;
    // (four steps of a wave = eight distance loads per lane in flight, unconditional and clamped, as for the window above)
    for (int base0 = (int)(tid & ~63u); base0 < win * row_cells; base0 += STEPS * (int)blockDim.x) {
      uint32_t dp[STEPS], dg[STEPS];
      bool in_map[STEPS];
#pragma unroll
      for (int u = 0; u < STEPS; ++u) {
        const int idx = min(base0 + u * (int)blockDim.x + (int)(tid & 63u), win * row_cells - 1);
        const int y = idx / row_cells, lx = idx - y * row_cells;
        const int gx = wx0 + lx, gy = wy0 + y;
        in_map[u] = lx < win && gx >= 0 && gy >= 0 && gx < (int)g.nx && gy < (int)g.ny;
        const uint32_t cell = (uint32_t)(min(max(gy, 0), (int)g.ny - 1)) * g.nx + (uint32_t)min(max(gx, 0), (int)g.nx - 1);
        dp[u] = dpath[cell];
        dg[u] = dgoal[cell];
      }
#pragma unroll
      for (int u = 0; u < STEPS; ++u) {
        const int base = base0 + u * (int)blockDim.x;
        if (base < win * row_cells) {  // (wave-uniform)
          const int idx = base + (int)(tid & 63u);
          unsigned long long mp, mg;
          gridScreenBits(pl, in_map[u] && idx < win * row_cells, dp[u], dg[u], mp, mg);
          if ((tid & 63u) == 0) {
            const int w = idx >> 5;  // linear word index y * nw + j; a wave covers two words (possibly of two rows)
            s_fb[4 * w + 2] = (uint32_t)mp;
            s_fb[4 * w + 3] = (uint32_t)mg;
            if (w + 1 < win * nw) {
              s_fb[4 * (w + 1) + 2] = (uint32_t)(mp >> 32);
              s_fb[4 * (w + 1) + 3] = (uint32_t)(mg >> 32);
            }
          }
        }
      }
    }
  }
}
__device__ __forceinline__ void walkOrder(const PlannerDev& pl, const ScoreRobot& r, uint8_t* s_win) {
  if (pl.cfg.allow_unknown != 0) {
    __syncthreads();
    for (int i = threadIdx.x; i < r.win * r.win; i += blockDim.x) {
      const uint8_t cc = s_win[i];
      if (cc >= 254) s_win[i] = cc ^ 1u;
    }
  }
}
__device__ __forceinline__ void buildScreens(const PlannerDev& pl, const ScoreRobot& r, uint8_t* s_dyn, uint32_t* s_ba) {
  buildFootprintScreens<true>(pl, r, s_dyn, s_ba);
  buildGridScreens<4>(pl, r, reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes));
  walkOrder(pl, r, s_dyn);
}

// ---- stage (the tables, use_tables: use_dwa && discretize_by_time, k_score_prep_tab only): per-(v_theta sample, step) heading, trig and
// rotated footprint, all tab_nth v_theta rows, behind the screens
__device__ __forceinline__ void buildTables(const PlannerDev& pl, const ScoreRobot& r, const double* s_fp, const float (*s_axis)[kMaxAxis], uint8_t* s_dyn) {
  const uint32_t tid = threadIdx.x;
  const navgpu_dwa_config& c = pl.cfg;
  const navgpu_robot_state& st = r.st;
  const uint32_t nfp = r.nfp;
  const int K = (int)pl.tab_steps;
  const int tnfp = (int)pl.tab_nfp;
  const int nth_s = r.cnt[2];
  const int lrows = (int)pl.tab_nth;
  double* s_trig = reinterpret_cast<double*>(s_dyn + r.win_bytes + score_bits_bytes(r.win));  // [rows][K][4] cs, sn, cs2, sn2
  double* s_rot = s_trig + (size_t)lrows * K * 4;                                              // [rows][K][tnfp][2]
  float* s_th = reinterpret_cast<float*>(s_rot + (size_t)lrows * K * tnfp * 2);                // [rows][K]
  __syncthreads();  // s_axis, s_fp staged
  const double dt_t = c.sim_time / K;
  for (int t = tid; t < nth_s; t += blockDim.x) {  // (a workgroup may have fewer lanes than there are v_theta samples)
    float pth = st.pos[2];
    const float vth = s_axis[2][t];
    for (int k = 0; k < K; ++k) {
      s_th[t * K + k] = pth;
      pth = (float)(pth + vth * dt_t);  // computeNewPositions :258
    }
  }
  __syncthreads();
  for (int e = tid; e < nth_s * K; e += blockDim.x) {
    const double th = s_th[e];
    double sn, cs, sn2, cs2;
    sincos(th, &sn, &cs);
    sincos(M_PI_2 + th, &sn2, &cs2);
    s_trig[4 * e] = cs;
    s_trig[4 * e + 1] = sn;
    s_trig[4 * e + 2] = cs2;
    s_trig[4 * e + 3] = sn2;
    for (int v = 0; v < (int)nfp && v < tnfp; ++v) {
      const double sx = s_fp[2 * v], sy = s_fp[2 * v + 1];
      s_rot[(e * tnfp + v) * 2] = sx * cs - sy * sn;      // world_model.h:72-73
      s_rot[(e * tnfp + v) * 2 + 1] = sx * sn + sy * cs;
    }
  }
}

// ---- stage: the LDS image as 16-byte words, [0, prep_bytes), to the robot's slot of pl.prep
__device__ __forceinline__ void storeImage(const PlannerDev& pl, const ScoreRobot& r, const uint8_t* s_dyn) {
  uint4* img = reinterpret_cast<uint4*>(pl.prep + (size_t)r.inst * pl.prep_stride);
  const uint4* lds = reinterpret_cast<const uint4*>(s_dyn);
  const uint32_t n16 = pl.prep_bytes >> 4;
  for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) img[i] = lds[i];
}

// ---- stage (the sweep's image only): the sweep's per-robot scalars and the reject bytes of the (vx, vy) pairs, behind the image.
// What every lane of the sweep launch would otherwise work out again: the robot's scalars (two fp64 divisions, a ceil)
// and the generator's reject tests of the (vx, vy) pairs (a compensated fp64 square root each).
// In two parts: the free distance and start_fail (aux[7], aux[8]) read the path and goal screens, the rest (aux[0..6], the reject
// bytes) does not.  storeSweepScalars is both.
__device__ __forceinline__ uint8_t* sweepRejectBytes(const PlannerDev& pl, uint32_t inst) {
  return pl.prep + (size_t)inst * pl.prep_stride + score_prep_reject_offset(pl);
}
__device__ __forceinline__ int32_t* sweepAux(const PlannerDev& pl, uint32_t inst) { return reinterpret_cast<int32_t*>(sweepRejectBytes(pl, inst) - kScoreAuxBytes); }
// s_fb: the robot's screens [win][nw][4]; s_min: one LDS word
__device__ __forceinline__ void storeFreeDistance(const PlannerDev& pl, const ScoreRobot& r, const uint32_t* s_fb, int* s_min) {
  const uint32_t tid = threadIdx.x;
  const navgpu_dwa_config& c = pl.cfg;
  const int win = r.win, nw = r.nw;
  int32_t* aux = sweepAux(pl, r.inst);
  // d0: how far (Euclidean, cells, rounded down) from the robot's own cell - the window's centre - the nearest cell lies at which ANY screen is
  // set (or the window ends).  A trajectory point fewer cells away than that passes every screen whatever else: the sweep skips
  // its worldToMap and look-up for as many steps as the sample's speed cannot cover d0 cells in (k_score_sweep).
  // The path / goal screen at the robot's own cell decides those critics for EVERY sample at step 0 (all rollouts start there):
  // start_fail = 4 (the path critic fails there; the goal critic, later in the list, no longer counts either) or 5 (the goal
  // critic does - e.g. a goal inside an inflated wall, 17 % of the benchmark's robots) or 0.  The distance is taken over the
  // screens that still count after that.
  const int c0 = win / 2;
  const uint32_t w_c0 = (uint32_t)(c0 * nw + (c0 >> 5));
  const int start_fail = ((s_fb[4 * w_c0 + 2] >> (c0 & 31)) & 1u) ? 4 : (((s_fb[4 * w_c0 + 3] >> (c0 & 31)) & 1u) ? 5 : 0);
  if (tid == 0) s_min[0] = (win / 2) * (win / 2);  // (squared: the distance is Euclidean - a pose moves |v| dt whatever its bearing)
  __syncthreads();
  {
    int dmin = win * win;
    for (int it = tid; it < win * nw; it += blockDim.x) {
      const int y = it / nw, j = it - y * nw;
      uint32_t m = (c.sum_scores ? s_fb[4 * it] : s_fb[4 * it + 1]) | (start_fail == 4 ? 0u : s_fb[4 * it + 2]) | (start_fail != 0 ? 0u : s_fb[4 * it + 3]);
      const int dy = y > c0 ? y - c0 : c0 - y;
      // the set cell nearest to column c0: the lowest set bit at or right of it, the highest left of it (no loop over the bits)
      const int p = c0 - 32 * j;  // c0's bit position in this word (may lie outside it)
      const uint32_t right = p <= 0 ? m : (p >= 32 ? 0u : m & (0xFFFFFFFFu << p)), left = m & ~right;
      if (right) dmin = min(dmin, (32 * j + __ffs(right) - 1 - c0) * (32 * j + __ffs(right) - 1 - c0) + dy * dy);
      if (left) dmin = min(dmin, (c0 - (32 * j + 31 - __clz(left))) * (c0 - (32 * j + 31 - __clz(left))) + dy * dy);
    }
    atomicMin(&s_min[0], dmin);
  }
  __syncthreads();
  if (tid == 0) {
    aux[7] = (int)floor(sqrt((double)s_min[0]));
    aux[8] = start_fail;
  }
}
// The three limits the sweep's scalars take from the robot's record.  Loaded where a workgroup begins, beside its other per-robot
// loads, and handed down: read where they are used - at the very end of the image build, which is the tail of the wavefront launch
// when it runs there (scorePrepFree) - the loads' latency would be that launch's.
struct SweepLimits {
  double min_trans_vel, max_trans_vel, min_rot_vel;
};
__device__ __forceinline__ SweepLimits sweepLimits(const PlannerDev& pl, uint32_t inst) {
  const RobotLimits& l = pl.limits[inst];
  return SweepLimits{l.min_trans_vel, l.max_trans_vel, l.min_rot_vel};
}
__device__ __forceinline__ void storeSweepRobotScalars(const PlannerDev& pl, const ScoreRobot& r, const float (*s_axis)[kMaxAxis], const SweepLimits& lim) {
  const uint32_t tid = threadIdx.x;
  const navgpu_dwa_config& c = pl.cfg;
  const Geom& g = r.g;
  const int32_t* cnt = r.cnt;
  const uint32_t inst = r.inst;
  const int win = r.win, wx0 = r.wx0, wy0 = r.wy0;
  uint8_t* rej = sweepRejectBytes(pl, inst);
  int32_t* aux = sweepAux(pl, inst);
  if (tid == 0) {
    const double inv_res = pl.inv_res, fpd = c.forward_point_distance;
    const bool en_fwd = pl.scale_goal != 0 || (pl.align_on[inst] && pl.scale_path != 0);  // goal_front or alignment critic on
    // the forward point (x + fpd cos, y + fpd sin) stays on the map whenever the centre cell is this many cells away from
    // every border; only then may a step skip its worldToMap
    const uint32_t fwd_margin = (uint32_t)fmin(ceil(fabs(fpd) * inv_res) + 1.0, 1.0e6);
    const bool fwd_screen = !en_fwd || (2u * fwd_margin < g.nx && 2u * fwd_margin < g.ny);
    const uint32_t fwd_lo = en_fwd ? fwd_margin : 0u, fwd_nx = g.nx - 2u * fwd_lo, fwd_ny = g.ny - 2u * fwd_lo;
    // the forward-margin test is only needed when the LDS window reaches into the margin band of the map
    const bool need_margin = !((uint32_t)wx0 - fwd_lo < fwd_nx && (uint32_t)(wx0 + win - 1) - fwd_lo < fwd_nx && (uint32_t)wy0 - fwd_lo < fwd_ny &&
                               (uint32_t)(wy0 + win - 1) - fwd_lo < fwd_ny);
    aux[0] = wx0;
    aux[1] = wy0;
    aux[2] = (int32_t)fwd_lo;
    aux[3] = (int32_t)fwd_nx;
    aux[4] = (int32_t)fwd_ny;
    aux[5] = need_margin ? 1 : 0;
    aux[6] = fwd_screen ? 1 : 0;
    *reinterpret_cast<double*>(aux + kSweepAuxMinRot) = lim.min_rot_vel;  // the v_theta half of the reject tests, for the sweep's lanes
  }
  // generateTrajectory's reject tests (simple_trajectory_generator.cpp:193-200), the part that depends on (vx, vy) only:
  // bit 0: vmag + eps < min_trans_vel (rejects together with the v_theta half), bit 1: vmag - eps > max_trans_vel
  const int nyv = max(cnt[1], 1), nxyv = cnt[0] * cnt[1];
  for (int i = tid; i < nxyv; i += blockDim.x) {
    const int ix = i / nyv, iy = i - ix * nyv;
    const double vmag = hyp2((double)s_axis[0][ix], (double)s_axis[1][iy]);
    const double eps = 1e-4;
    rej[i] = (uint8_t)(((lim.min_trans_vel >= 0 && vmag + eps < lim.min_trans_vel) ? 1 : 0) | ((lim.max_trans_vel >= 0 && vmag - eps > lim.max_trans_vel) ? 2 : 0));
  }
}
__device__ __forceinline__ void storeSweepScalars(const PlannerDev& pl, const ScoreRobot& r, const float (*s_axis)[kMaxAxis], int* s_cnt,
                                                  const uint8_t* s_dyn, const SweepLimits& lim) {
  storeFreeDistance(pl, r, reinterpret_cast<const uint32_t*>(s_dyn + r.win_bytes), s_cnt);
  storeSweepRobotScalars(pl, r, s_axis, lim);
}

// ---- scorePrepFree: the part of k_score_prep_tab's image that reads neither the path nor the goal grid - the window bytes, the
// footprint screens, the heading tables, aux[0..6] and the reject bytes - with words 2 and 3 of every screen cell stored as zero;
// k_score_prep_grids completes it (those words, aux[7], aux[8]).  For a workgroup of any whole number of waves: it also runs as extra
// workgroups of the wavefront launch (k_bfs_rows), whose own workgroups it does not have to wait for.
// s_dyn: score_prep_free_lds_bytes(pl) of LDS: the image, the dilation's scratch, and the footprint, axis samples and counters
// that the kernels of planner_score.hip keep in static LDS.
__host__ __device__ inline size_t score_prep_free_tail_bytes() { return 2 * kMaxFootprint * sizeof(double) + 3 * kMaxAxis * sizeof(float) + 16; }
__device__ __forceinline__ void scorePrepFree(const PlannerDev& pl, uint32_t inst, uint8_t* s_dyn) {
  ScoreRobot r = scoreRobot(pl, inst);
  const SweepLimits lim = sweepLimits(pl, inst);
  uint32_t* s_ba = reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes + score_bits_bytes(r.win) + pl.tab_bytes);
  double* s_fp = reinterpret_cast<double*>(reinterpret_cast<uint8_t*>(s_ba) + score_scratch_bytes(r.win));
  float(*s_axis)[kMaxAxis] = reinterpret_cast<float(*)[kMaxAxis]>(s_fp + 2 * kMaxFootprint);
  int* s_cnt = reinterpret_cast<int*>(s_axis + 3);
  stageInputs<false>(pl, r, s_fp, s_axis, s_cnt, s_dyn);
  __syncthreads();
  buildFootprintScreens<false>(pl, r, s_dyn, s_ba);
  walkOrder(pl, r, s_dyn);
  buildTables(pl, r, s_fp, s_axis, s_dyn);
  __syncthreads();
  storeImage(pl, r, s_dyn);
  storeSweepRobotScalars(pl, r, s_axis, lim);
}

}  // namespace navgpu
