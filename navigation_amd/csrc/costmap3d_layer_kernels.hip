// costmap_3d's layered map update on the bit volumes of a navgpu_costmap3d handle (include/navgpu_costmap3d_layers.h):
// k_c3d_cloud and k_c3d_static2d write a layer's new cells into its next plane set, k_c3d_layer_swap makes that set current and
// accumulates the changed plane, k_c3d_combine is LayeredCostmap3D::updateMap with the projection into the 2-D layer, and
// k_c3d_costs2d is Costmap3DTo2DLayer::updateCosts.  A cell is one-hot in three planes (LETHAL, NONLETHAL, FREE), so every rule
// is a bitwise operation on column words.  A tile is 64 consecutive column words of a row: a wave.  The swap and the combine
// look a tile's bit up and leave before they load a word of a tile that no cloud touched (all_tiles, tool builds: they do not).
// All geometry is fp64 under -ffp-contract=off: tests/costmap3d_layers_ref.py evaluates the same expressions in numpy.
#include "navgpu_costmap3d.h"

namespace navgpu {
namespace {

using ull = unsigned long long;

__device__ __forceinline__ ull* words(uint64_t* p) { return reinterpret_cast<ull*>(p); }
__device__ __forceinline__ uint32_t tileOf(const C3dLayersDev& ly, uint32_t x, uint32_t y) { return y * ly.tpr + (x >> 6); }
__device__ __forceinline__ bool tileBit(const uint32_t* map, uint32_t tile) { return (map[tile >> 5] >> (tile & 31)) & 1u; }
// (a stale read only costs a second atomic: the bit is never cleared while a launch sets it)
__device__ __forceinline__ void setTileBit(uint32_t* map, uint32_t tile) {
  if (!tileBit(map, tile)) atomicOr(map + (tile >> 5), 1u << (tile & 31));
}
// octomap's coordToKey less the origin's key; false: not finite or off the axis' extent
__device__ __forceinline__ bool cellOf(double c, double inv_res, int64_t ok, uint32_t size, uint32_t* cell) {
  const double f = floor(c * inv_res);
  if (!(fabs(f) < 4.0e18)) return false;  // (NaN too)
  const int64_t k = (int64_t)f - ok;
  if (k < 0 || k >= (int64_t)size) return false;
  *cell = (uint32_t)k;
  return true;
}
// one new cell of class cls into the next set of a layer
__device__ __forceinline__ void markCell(const C3dDev& d, const C3dLayersDev& ly, uint32_t inst, uint32_t slot, uint32_t next, uint32_t x, uint32_t y,
                                         uint32_t z, uint32_t cls) {
  atomicOr(words(ly.set(inst, slot, next, d.cols) + (size_t)cls * d.cols) + (size_t)y * d.sx + x, 1ull << z);
  setTileBit(ly.occOf(inst, slot, next), tileOf(ly, x, y));
}
// the lanes of a wave that dropped their item: one add per wave
__device__ __forceinline__ void countClipped(bool clipped, uint32_t* counter) {
  const ull m = __ballot(clipped);
  if (m && (threadIdx.x & 63) == (uint32_t)__ffsll((long long)m) - 1) atomicAdd(counter, (uint32_t)__popcll(m));
}

// A lane per point; blockIdx.y is the cloud.  PointCloudLayer3D::pointCloudCallback up to new_cells (point_cloud_layer_3d.cpp:171-216)
__global__ __launch_bounds__(256) void k_c3d_cloud(C3dDev d, C3dLayersDev ly, const C3dCloudRec* clouds, const float* points, uint32_t* clipped) {
  const C3dCloudRec& c = clouds[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.n_points) return;
  const uint32_t stride = c.has_intensity ? 4u : 3u;
  const float* p = points + (size_t)(c.first_point + i) * stride;
  const double x = p[0], y = p[1], z = p[2];
  // pcl::transformPointCloud with an Affine3d: fp64, stored as float
  const float wx = (float)(c.tf[0] * x + c.tf[1] * y + c.tf[2] * z + c.tf[9]);
  const float wy = (float)(c.tf[3] * x + c.tf[4] * y + c.tf[5] * z + c.tf[10]);
  const float wz = (float)(c.tf[6] * x + c.tf[7] * y + c.tf[8] * z + c.tf[11]);
  uint32_t cls = kC3dL;
  if (c.has_intensity) {  // pointIntensityToCost (:159-169), in float
    const float intensity = p[3];
    if (intensity >= c.lethal_intensity) cls = kC3dL;
    else if (intensity <= c.free_intensity) cls = kC3dF;
    else {
      const float cost = ((intensity - c.free_intensity) / (c.lethal_intensity - c.free_intensity)) * (10.0f - -10.0f) + -10.0f;
      cls = cost >= 10.0f ? kC3dL : cost <= -10.0f ? kC3dF : kC3dN;  // (NaN: neither comparison holds)
    }
  }
  uint32_t cx = 0, cy = 0, cz = 0;
  const bool inside = cellOf((double)wx, ly.inv_res, c.ok[0], d.sx, &cx) && cellOf((double)wy, ly.inv_res, c.ok[1], d.sy, &cy) &&
                      cellOf((double)wz, ly.inv_res, c.ok[2], d.sz, &cz);
  if (inside) markCell(d, ly, c.instance, c.slot, c.next, cx, cy, cz, cls);
  countClipped(!inside, clipped + blockIdx.y);
}

// A lane per grid cell.  Static2DLayer3D::occupancyGridCallback up to new_cells (static_2d_layer_3d.cpp:256-273)
__global__ __launch_bounds__(256) void k_c3d_static2d(C3dDev d, C3dLayersDev ly, const C3dGridRec* rec, const int8_t* grid, uint32_t* clipped) {
  const C3dGridRec& g = *rec;
  const size_t cell = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= (size_t)g.width * g.rows) return;
  const uint32_t i = (uint32_t)(cell % g.width), j = (uint32_t)(cell / g.width);
  const int v = grid[(size_t)j * g.width + i];
  int cls = -1;  // occupancyGridToCost (:189-199); -1: UNKNOWN, no cell
  if (v < 0) cls = g.unknown_to_lethal ? (int)kC3dL : -1;
  else cls = v >= g.threshold ? (int)kC3dL : (int)kC3dF;
  const double res = d.res;
  const double x = g.origin_x + i * res + res / 2.0, y = g.origin_y + j * res + res / 2.0;
  uint32_t cx = 0, cy = 0, cz = 0;
  const bool inside = cellOf(x, ly.inv_res, g.ok[0], d.sx, &cx) && cellOf(y, ly.inv_res, g.ok[1], d.sy, &cy) && cellOf(g.height, ly.inv_res, g.ok[2], d.sz, &cz);
  if (cls >= 0 && inside) markCell(d, ly, g.instance, g.slot, g.next, cx, cy, cz, (uint32_t)cls);
  countClipped(cls >= 0 && !inside, clipped);
}

// A wave per (pair, tile).  mode 0: the next set becomes one-hot (the highest class per cell, point_cloud_layer_3d.cpp:210-214),
// changed |= old ^ new (:218-241), the old set is emptied to be the next scratch.  mode 1: changed |= present (touch).
__global__ __launch_bounds__(256) void k_c3d_layer_swap(C3dDev d, C3dLayersDev ly, const uint32_t* pairs3, int32_t mode) {
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= ly.tiles) return;
  const uint32_t inst = pairs3[3 * blockIdx.y], slot = pairs3[3 * blockIdx.y + 1], next = pairs3[3 * blockIdx.y + 2];
  uint32_t* occ_new = ly.occOf(inst, slot, next);
  uint32_t* occ_old = ly.occOf(inst, slot, next ^ 1u);
  const bool in_new = tileBit(occ_new, tile), in_old = tileBit(occ_old, tile);
  if (mode == 1 ? !(in_old || ly.all_tiles) : !(in_new || in_old || ly.all_tiles)) return;  // (wave-uniform)
  const uint32_t y = tile / ly.tpr, x = (tile % ly.tpr) * 64 + lane;
  const bool live = x < d.sx;
  const size_t w = (size_t)y * d.sx + x;
  uint64_t* pn = ly.set(inst, slot, next, d.cols);
  uint64_t* po = ly.set(inst, slot, next ^ 1u, d.cols);
  uint64_t diff = 0;
  if (live && mode == 1) {
    diff = po[w] | po[d.cols + w] | po[2 * (size_t)d.cols + w];
  } else if (live) {
    const uint64_t nl = pn[w];
    const uint64_t nn = pn[d.cols + w] & ~nl;
    const uint64_t nf = pn[2 * (size_t)d.cols + w] & ~(nl | nn);
    pn[d.cols + w] = nn;
    pn[2 * (size_t)d.cols + w] = nf;
    const uint64_t ol = po[w], on = po[d.cols + w], of = po[2 * (size_t)d.cols + w];
    diff = (ol ^ nl) | (on ^ nn) | (of ^ nf);
    if (ol | on | of) po[w] = po[d.cols + w] = po[2 * (size_t)d.cols + w] = 0;
  }
  if (diff) ly.changed[((size_t)inst * ly.nc + slot) * d.cols + w] |= diff;
  const bool any = __ballot(diff != 0) != 0;
  if (lane == 0) {
    if (any) setTileBit(ly.dirty + (size_t)inst * ly.tw, tile);
    if (mode == 0 && in_old) atomicAnd(occ_old + (tile >> 5), ~(1u << (tile & 31)));
  }
}

__device__ __forceinline__ bool inBox(const int32_t* box, int32_t x, int32_t y) { return x >= box[0] && x <= box[1] && y >= box[2] && y <= box[3]; }
// the column's centre inside the cylinder (cylinder_clearing_layer_3d.cpp:116-131): keyToCoord less the robot's position
__device__ __forceinline__ bool inCylinder(const int32_t* box, double rx, double ry, double r, double res, const int64_t* ok, int32_t x, int32_t y) {
  if (!inBox(box, x, y)) return false;
  const double dx = ((double)(ok[0] + x) + 0.5) * res - rx, dy = ((double)(ok[1] + y) + 0.5) * res - ry;
  return dx * dx + dy * dy <= r * r;
}

// A wave per (listed instance, tile), a lane per column word: LayeredCostmap3D::updateMap (layered_costmap_3d.cpp:60-165) and the
// projection of the columns inside bounds (costmap_3d_to_2d_layer.cpp:196-232, 246-277)
__global__ __launch_bounds__(256) void k_c3d_combine(C3dDev d, C3dLayersDev ly, C3dUpdate u) {
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= ly.tiles) return;
  const uint32_t k = blockIdx.y, inst = u.instances[k];
  const uint32_t y = tile / ly.tpr, x0 = (tile % ly.tpr) * 64, x = x0 + lane;
  const bool full = u.full[k] != 0;
  uint32_t* dirty = ly.dirty + (size_t)inst * ly.tw;
  const bool is_dirty = tileBit(dirty, tile);
  const C3dCylRec* cyl = u.cyl + (size_t)k * u.n_cyl;
  bool wanted = full || is_dirty || ly.all_tiles;
  for (uint32_t c = 0; c < u.n_cyl && !wanted; ++c) {  // a cylinder's key box meets the tile's columns (wave-uniform)
    const int32_t xa = (int32_t)x0, xb = (int32_t)x0 + 63, yy = (int32_t)y;
    wanted = (cyl[c].has_cur && cyl[c].cbox[0] <= xb && cyl[c].cbox[1] >= xa && cyl[c].cbox[2] <= yy && cyl[c].cbox[3] >= yy) ||
             (cyl[c].has_prev && cyl[c].pbox[0] <= xb && cyl[c].pbox[1] >= xa && cyl[c].pbox[2] <= yy && cyl[c].pbox[3] >= yy);
  }
  if (!wanted) return;
  const uint64_t all = d.sz >= 64 ? ~0ull : (1ull << d.sz) - 1;
  const int64_t* ok = u.ok + 3 * (size_t)k;
  uint64_t bounds = 0;
  if (x < d.sx) {
    const size_t w = (size_t)y * d.sx + x;
    // updateBounds of every layer: the changed cells (costmap_layer_3d.cpp:66-74), the cylinders' previous and current sets
    uint64_t cur_cyl = 0;  // bit c: inside cylinder layer c's current set
    if (full) bounds = all;
    if (is_dirty || ly.all_tiles)
      for (uint32_t s = 0; s < ly.nc; ++s) {
        uint64_t* ch = ly.changed + ((size_t)inst * ly.nc + s) * d.cols + w;
        const uint64_t v = *ch;
        if (v) {
          bounds |= v;
          *ch = 0;
        }
      }
    for (uint32_t c = 0; c < u.n_cyl; ++c) {
      if (cyl[c].has_prev && inCylinder(cyl[c].pbox, cyl[c].px, cyl[c].py, cyl[c].r, d.res, ok, (int32_t)x, (int32_t)y)) bounds = all;
      if (cyl[c].has_cur && inCylinder(cyl[c].cbox, cyl[c].cx, cyl[c].cy, cyl[c].r, d.res, ok, (int32_t)x, (int32_t)y)) {
        bounds = all;
        cur_cyl |= 1ull << c;
      }
    }
    if (bounds) {
      uint64_t* mp = d.planes + (size_t)inst * 2 * d.cols + w;
      uint64_t* fp = ly.free_plane + (size_t)inst * d.cols + w;
      const uint64_t keep = ~bounds;
      uint64_t L = mp[0] & keep, N = mp[d.cols] & keep, F = *fp & keep;  // the cells being updated are deleted (:127)
      for (uint32_t r = 0; r < u.n_layers; ++r) {
        const C3dLayerRule rule = u.rules[r];
        if (!rule.enabled) continue;
        if (rule.kind == NAVGPU_C3D_LAYER_CYLINDER_CLEARING) {
          if ((cur_cyl >> rule.index) & 1ull) L = N = F = 0;
          continue;
        }
        if (rule.method == NAVGPU_C3D_COMBINE_NOTHING) continue;
        const uint64_t* lp = ly.set(inst, (uint32_t)rule.index, u.cur[(size_t)k * ly.nc + rule.index], d.cols) + w;
        const uint64_t l = lp[0] & bounds, n = lp[d.cols] & bounds, f = lp[2 * (size_t)d.cols] & bounds;
        if (rule.method == NAVGPU_C3D_COMBINE_OVERWRITE) {
          const uint64_t away = ~(l | n | f);
          L = (L & away) | l;
          N = (N & away) | n;
          F = (F & away) | f;
        } else if (rule.method == NAVGPU_C3D_COMBINE_MAXIMUM) {
          L |= l;
          N = (N | n) & ~L;
          F = (F | f) & ~(L | N);
        } else {  // IfUnknown: only where the master has no node
          const uint64_t absent = ~(L | N | F);
          L |= l & absent;
          N |= n & absent;
          F |= f & absent;
        }
      }
      mp[0] = L;
      mp[d.cols] = N;
      *fp = F;
      ly.layer2d[(size_t)inst * d.cols + w] = L ? 254 : N ? (uint8_t)ly.nonlethal_cost_2d : F ? 0 : 255;
    }
  }
  // the 2-D bounds of the columns touched: the wave's lanes are consecutive x of one row
  const ull m = __ballot(bounds != 0);
  if (lane == 0) {
    if (is_dirty) atomicAnd(dirty + (tile >> 5), ~(1u << (tile & 31)));
    if (m) {
      int32_t* box = u.box + 4 * (size_t)k;
      atomicMin(box + 0, (int32_t)x0 + (__ffsll((long long)m) - 1));
      atomicMin(box + 1, (int32_t)y);
      atomicMax(box + 2, (int32_t)x0 + 63 - __clzll((long long)m));
      atomicMax(box + 3, (int32_t)y);
    }
  }
}

// A lane per cell of the map, blockIdx.y the listed instance: CostmapLayer::updateWithMax / updateWithOverwrite (costmap_layer.cpp:62-124)
__global__ __launch_bounds__(256) void k_c3d_costs2d(C3dDev d, C3dLayersDev ly, C3dCosts2d c) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (cell >= d.cols) return;
  const uint32_t x = cell % d.sx, y = cell / d.sx;
  const int32_t* box = c.boxes + 4 * (size_t)k;
  if ((int32_t)x < box[0] || (int32_t)x >= box[2] || (int32_t)y < box[1] || (int32_t)y >= box[3]) return;
  const uint32_t inst = c.instances[k];
  const uint8_t v = ly.layer2d[(size_t)inst * d.cols + (size_t)y * d.sx + x];
  if (v == 255) return;  // NO_INFORMATION
  uint8_t* m = c.grid + (size_t)inst * c.stride + (size_t)y * d.sx + x;
  if (c.use_maximum) {
    const uint8_t old = *m;
    if (old == 255 || old < v) *m = v;
  } else {
    *m = v;
  }
}

__global__ void k_c3d_fill_u8(uint8_t* p, uint8_t v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

}  // namespace

void launch_c3d_cloud(const C3dDev& d, const C3dLayersDev& ly, const C3dCloudRec* clouds, uint32_t n_clouds, uint32_t max_points, const float* points,
                      uint32_t* clipped, hipStream_t stream) {
  if (!max_points) return;
  for (uint32_t first = 0; first < n_clouds; first += 65535u) {  // (gridDim.y)
    const uint32_t count = n_clouds - first < 65535u ? n_clouds - first : 65535u;
    hipLaunchKernelGGL(k_c3d_cloud, dim3((max_points + 255) / 256, count), dim3(256), 0, stream, d, ly, clouds + first, points, clipped + first);
  }
}

void launch_c3d_static2d(const C3dDev& d, const C3dLayersDev& ly, const C3dGridRec* rec, size_t cells, const int8_t* grid, uint32_t* clipped,
                         hipStream_t stream) {
  hipLaunchKernelGGL(k_c3d_static2d, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, stream, d, ly, rec, grid, clipped);
}

void launch_c3d_layer_swap(const C3dDev& d, const C3dLayersDev& ly, const uint32_t* pairs3, uint32_t n_pairs, int32_t mode, hipStream_t stream) {
  for (uint32_t first = 0; first < n_pairs; first += 65535u) {
    const uint32_t count = n_pairs - first < 65535u ? n_pairs - first : 65535u;
    hipLaunchKernelGGL(k_c3d_layer_swap, dim3((ly.tiles + 3) / 4, count), dim3(256), 0, stream, d, ly, pairs3 + 3 * (size_t)first, mode);
  }
}

void launch_c3d_combine(const C3dDev& d, const C3dLayersDev& ly, const C3dUpdate& u, hipStream_t stream) {
  for (uint32_t first = 0; first < u.n; first += 65535u) {
    C3dUpdate part = u;
    part.n = u.n - first < 65535u ? u.n - first : 65535u;
    part.instances += first;
    part.cur += (size_t)first * ly.nc;
    part.full += first;
    part.ok += 3 * (size_t)first;
    part.cyl += (size_t)first * u.n_cyl;
    part.box += 4 * (size_t)first;
    hipLaunchKernelGGL(k_c3d_combine, dim3((ly.tiles + 3) / 4, part.n), dim3(256), 0, stream, d, ly, part);
  }
}

void launch_c3d_costs2d(const C3dDev& d, const C3dLayersDev& ly, const C3dCosts2d& c, hipStream_t stream) {
  for (uint32_t first = 0; first < c.n; first += 65535u) {
    C3dCosts2d part = c;
    part.n = c.n - first < 65535u ? c.n - first : 65535u;
    part.instances += first;
    part.boxes += 4 * (size_t)first;
    hipLaunchKernelGGL(k_c3d_costs2d, dim3((d.cols + 255) / 256, part.n), dim3(256), 0, stream, d, ly, part);
  }
}

void launch_c3d_fill_u8(uint8_t* p, uint8_t v, size_t n, hipStream_t stream) {
  if (!n) return;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_c3d_fill_u8, dim3((uint32_t)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, p, v, n);
}

}  // namespace navgpu
