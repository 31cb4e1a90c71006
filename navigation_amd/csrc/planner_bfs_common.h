// What the three MapGrid wavefront kernels (k_bfs_rows, k_bfs_rows2: planner_bfs_rows.hip; k_bfs_global: planner_bfs.hip)
// do alike around their level loops: seeds from the plan, the robot's region, distance stores, trace stamps.  gfx950 only.
#pragma once
#include "planner_common.h"

namespace navgpu {

// The seed cells of wavefront `which` of robot `inst`, from its plan (adjustPlanResolution + setTargetCells | setLocalGoal,
// map_grid.cpp:160-187, 190-233): every lane of the workgroup takes a slice of the plan, `set(mx, my)` is called once per
// seed cell.  s_wave: 16 words of LDS.
template <typename Set>
__device__ __forceinline__ void bfsPlanSeeds(const PlannerDev& pl, const uint32_t inst, const int which, const Geom& g, const uint8_t* master,
                                             const uint32_t nx, const uint32_t tid, uint32_t* s_wave, Set&& set) {
  const uint32_t n = pl.plan_count[inst];
  const double* P = pl.plan + (size_t)inst * pl.max_plan * 2;
  const bool ovr = which == 2;
  const double lx = pl.front_last[2 * inst], ly = pl.front_last[2 * inst + 1];
  const uint32_t chunk = (n + blockDim.x - 1) / blockDim.x;
  const uint32_t i0 = min(n, tid * chunk), i1 = min(n, i0 + chunk);
  uint32_t mine = 0;
  for (uint32_t i = i0; i < i1; ++i) mine += adjustedPoints(P, i, lx, ly, ovr, n, g.res, true, [](uint32_t, double, double) {});
  uint32_t total;
  const uint32_t base = blockExclusiveScan1024(mine, s_wave, &total);
  auto valid = [&](double x, double y, uint32_t& cell) {
    uint32_t mx, my;
    if (!worldToMap(g, x, y, mx, my)) return false;
    cell = my * nx + mx;
    return master[cell] != kNoInfo;
  };
  uint32_t fmin_ = 0xFFFFFFFFu, b = base;
  for (uint32_t i = i0; i < i1; ++i)
    b += adjustedPoints(P, i, lx, ly, ovr, n, g.res, false, [&](uint32_t k, double x, double y) {
      uint32_t cell;
      if (valid(x, y, cell)) fmin_ = min(fmin_, b + k);
    });
  const uint32_t f = blockMin1024(fmin_, s_wave);
  if (f == 0xFFFFFFFFu) return;  // (uniform over the workgroup)
  uint32_t emin = total;
  b = base;
  for (uint32_t i = i0; i < i1; ++i)
    b += adjustedPoints(P, i, lx, ly, ovr, n, g.res, false, [&](uint32_t k, double x, double y) {
      uint32_t cell;
      if (b + k > f && !valid(x, y, cell)) emin = min(emin, b + k);
    });
  const uint32_t e = blockMin1024(emin, s_wave);
  b = base;
  for (uint32_t i = i0; i < i1; ++i)
    b += adjustedPoints(P, i, lx, ly, ovr, n, g.res, false, [&](uint32_t k, double x, double y) {
      const uint32_t idx = b + k;
      const bool seed = (which == 0) ? (idx >= f && idx < e) : (idx == e - 1);
      if (!seed) return;
      uint32_t cell;
      if (!valid(x, y, cell)) return;
      const uint32_t my = cell / nx;
      set(cell - my * nx, my);
    });
}

// The same cells as a list: in a cycle the k_samples launch in front of the wavefronts runs bfsPlanSeeds once per (robot,
// grid) and leaves the cells in pl.bfs_seed_cells (pl.bfs_seed_cap != 0 for both launches), so an item only scatters them.
// An entry is the cell's bit index in a [ny][Wr] bitmap, word << 5 | bit.  A list is not there when the launch has no
// k_samples in front of it (cap 0) or the cells did not fit (count kNoSeedList): then the item walks the plan itself.
struct BfsSeedList {
  const uint32_t* cells;
  uint32_t n;      // (uniform over the workgroup)
  uint32_t first;  // this lane's first entry, loaded ahead of the item's zeroing pass
  bool listed;
};
__device__ __forceinline__ BfsSeedList bfsSeedList(const PlannerDev& pl, const uint32_t inst, const int which, const uint32_t tid) {
  BfsSeedList l{pl.bfs_seed_cells + ((size_t)inst * 3 + which) * kSeedListMax, 0, 0, false};
  if (pl.bfs_seed_cap) l.n = __builtin_amdgcn_readfirstlane(pl.bfs_seed_count[(size_t)inst * 3 + which]);
  l.listed = pl.bfs_seed_cap != 0 && l.n <= kSeedListMax;
  if (l.listed && tid < l.n) l.first = l.cells[tid];
  return l;
}
// set(entry) once per cell of the list, every lane of the workgroup taking a slice
template <typename Set>
__device__ __forceinline__ void bfsListSeeds(const BfsSeedList& l, const uint32_t tid, Set&& set) {
  if (tid < l.n) set(l.first);
  for (uint32_t i = tid + blockDim.x; i < l.n; i += blockDim.x) set(l.cells[i]);
}

// The robot's region: its box grown by two cells (k_samples), in cells x0 .. x1, y0 .. y1 and bitmap words w0 .. w1, and
// whether its pockets are known (care_ok: pl.bfs_care holds the mask).  A search that is not bounded - the launch is not,
// or the robot has no box this cycle - has the whole map for a region and no pocket mask: nothing is ever "settled".
struct BfsRegion {
  int x0, x1, y0, y1, care_ok;
  bool bounded;
  int w0, w1;
};
// (uniform over the workgroup; the values go through readfirstlane, so the row sweeps keep them in SGPRs.)  Only a DWA
// cycle sets pl.bfs_bounded (navgpu_planner_cycle, three grids); the legacy planner's two-grid launch (tpLaunchGrids) and
// ensureCompleteGrids launch with a copy that has it cleared, so bfs_bounded alone is the condition for every kernel.
__device__ __forceinline__ BfsRegion bfsRegion(const PlannerDev& pl, const uint32_t inst) {
  BfsRegion r{0, -1, 0, -1, 0, false, 0, 0};
  if (pl.bfs_bounded) {
    const int4 bb = reinterpret_cast<const int4*>(pl.bfs_box)[2 * inst];
    r.x0 = __builtin_amdgcn_readfirstlane(bb.x);
    r.x1 = __builtin_amdgcn_readfirstlane(bb.y);
    r.y0 = __builtin_amdgcn_readfirstlane(bb.z);
    r.y1 = __builtin_amdgcn_readfirstlane(bb.w);
    r.care_ok = __builtin_amdgcn_readfirstlane(pl.bfs_box[8 * inst + 4]);
  }
  r.bounded = r.x1 >= r.x0 && r.y1 >= r.y0;
  if (!r.bounded) {
    r.x0 = 0;
    r.y0 = 0;
    r.x1 = (int)pl.nx - 1;
    r.y1 = (int)pl.ny - 1;
    r.care_ok = 0;
  }
  r.w0 = r.x0 >> 5;
  r.w1 = r.x1 >> 5;
  return r;
}
// groups of four words that hold words of the region
__device__ __forceinline__ uint32_t bfsRegionGroups(const BfsRegion& r) {
  uint32_t groups = 0;
  for (int j = r.w0; j <= r.w1; ++j) groups |= 1u << (j >> 2);
  return groups;
}
// the bits of bitmap word j that lie in columns x0 .. x1 (the stop test looks at the region's words through it)
__device__ __forceinline__ uint32_t bfsColMask(const int x0, const int x1, const int j) {
  const int c_lo = max(x0 - j * 32, 0), c_hi = min(x1 - j * 32, 31);
  return c_hi >= c_lo ? ((0xFFFFFFFFu >> (31 - c_hi)) & (0xFFFFFFFFu << c_lo)) : 0u;
}

// Distance `value` for the cells `cells` of the bitmap word whose first cell's distance is at word_base.  Two plain bit
// loops (every lane runs the longest one, so their bodies are kept to a find-first-bit, an address and a store): with rows
// that are whole 16-byte units (aligned4), whole aligned groups of four first - fronts that run along a row reach 32 cells
// of a word at once - then what is left, cell by cell.
__device__ __forceinline__ void bfsStoreCells(uint32_t* word_base, uint32_t cells, const uint32_t value, const bool aligned4) {
  if (aligned4) {
    uint32_t full = cells & (cells >> 1) & (cells >> 2) & (cells >> 3) & 0x11111111u;
    cells &= ~(full * 15u);
    const uint4 v4 = make_uint4(value, value, value, value);
    while (full) {
      const uint32_t bpos = (uint32_t)__ffs(full) - 1u;
      *reinterpret_cast<uint4*>(word_base + bpos) = v4;
      full &= full - 1;
    }
  }
  while (cells) {
    const uint32_t bpos = (uint32_t)__ffs(cells) - 1u;
    word_base[bpos] = value;
    cells &= cells - 1;
  }
}

// phase stamps of a row sweep's work item (tools/trace_bfs.py; pl.bfs_trace is null outside tool builds)
__device__ __forceinline__ void bfsStamp(const PlannerDev& pl, const uint32_t tid, const uint32_t item, const uint32_t slot) {
  if (pl.bfs_trace && tid == 0) pl.bfs_trace[(size_t)item * 8 + slot] = wall_clock64();
}
// the end of a search: the closing stamps, and the level count that orders the next cycle's dispatch
__device__ __forceinline__ void bfsFinish(const PlannerDev& pl, const uint32_t tid, const uint32_t inst, const int which, const uint32_t item, const uint32_t level) {
  if (pl.bfs_trace && tid == 0) {
    pl.bfs_trace[(size_t)item * 8 + 6] = wall_clock64();
    pl.bfs_trace[(size_t)item * 8 + 1] = wall_clock64() | ((unsigned long long)level << 48);
  }
  if (tid == 0 && pl.bfs_grids == 3) pl.bfs_levels[(size_t)inst * 3 + which] = level;
}

}  // namespace navgpu
