// Pruned octree leaves out of a navgpu_costmap3d handle's bit volumes and back into a layer (include/navgpu_costmap3d_publish.h,
// DESIGN 4ad).
//   k_c3d_export<false>  a workgroup per (listed instance, 64 x 64-column lattice-aligned block): counts the block's leaves
//   k_c3d_export_scan    one workgroup: the counts' exclusive prefix over the list, and each instance's ranges
//   k_c3d_export<true>   the same workgroups again: each writes its leaves at its offset, in order
//   k_c3d_shadow_copy    DELTA, once the host has seen that the counts fit: the shadow becomes the master
//   k_c3d_cells_raster   a lane per column of a leaf: the bounds and the value leaves into call-scoped scratch planes
//   k_c3d_cells_resolve  a wave per (message, tile): layer = (old & ~E) | (V & E), changed |= E, the tile bitmaps
// Pruning.  A block's column words of one plane stand in LDS (level 0).  Level L holds, per node of 2^L x 2^L columns, the mask of
// the levels z at which a full cube of edge 2^L starts, z on the lattice's 2^L grid: the AND of the four nodes below, then
// v & (v >> 2^(L-1)), then the mask of the aligned starts.  A node is a leaf iff it is full and its parent is not.  Everything is
// integers and bits; leaf positions come from counts and scans, so the output does not depend on the order workgroups run in.
#include "block_scan.h"
#include "navgpu_costmap3d.h"

namespace navgpu {
namespace {

using ull = unsigned long long;

constexpr uint32_t kLevels = 7;  // 0..6
// where a level's nodes start in the pyramid: 4096, 1024, 256, 64, 16, 4, 1 words
__device__ __forceinline__ constexpr uint32_t levelAt(uint32_t L) { return L == 0 ? 0u : L == 1 ? 4096u : L == 2 ? 5120u : L == 3 ? 5376u : L == 4 ? 5440u : L == 5 ? 5456u : 5460u; }
constexpr uint32_t kPyramidWords = 5461;

__device__ __forceinline__ bool tileBit(const uint32_t* map, uint32_t tile) { return (map[tile >> 5] >> (tile & 31)) & 1u; }

// the starts z with (okz + z) % 2^L == 0
__device__ __forceinline__ uint64_t alignedStarts(uint32_t L, int32_t okz) {
  const uint64_t period = L == 0 ? ~0ull : L == 1 ? 0x5555555555555555ull : L == 2 ? 0x1111111111111111ull : L == 3 ? 0x0101010101010101ull
                          : L == 4 ? 0x0001000100010001ull : L == 5 ? 0x0000000100000001ull : 1ull;
  return period << ((0u - (uint32_t)okz) & ((1u << L) - 1u));
}

// a column word of the master (plane 0 LETHAL, 1 NONLETHAL, 2 FREE) or of the shadow; zero off the window
__device__ __forceinline__ uint64_t masterWord(const C3dDev& d, const C3dLayersDev& ly, uint32_t inst, uint32_t plane, int32_t x, int32_t y) {
  if (x < 0 || y < 0 || x >= (int32_t)d.sx || y >= (int32_t)d.sy) return 0;
  const size_t w = (size_t)y * d.sx + (uint32_t)x;
  return plane < 2 ? d.planes[((size_t)inst * 2 + plane) * d.cols + w] : ly.free_plane[(size_t)inst * d.cols + w];
}
__device__ __forceinline__ uint64_t shadowWord(const C3dDev& d, const C3dExport& e, const C3dExportRec& r, uint32_t plane, int32_t x, int32_t y) {
  const int64_t xs = (int64_t)x + r.sd[0], ys = (int64_t)y + r.sd[1];
  if (xs < 0 || ys < 0 || xs >= (int64_t)d.sx || ys >= (int64_t)d.sy || r.sd[2] >= 64 || r.sd[2] <= -64) return 0;
  const uint64_t v = e.shadow[((size_t)r.instance * e.np + plane) * d.cols + (size_t)ys * d.sx + (size_t)xs];
  const uint64_t all = d.sz >= 64 ? ~0ull : (1ull << d.sz) - 1;
  return (r.sd[2] >= 0 ? v >> r.sd[2] : v << -r.sd[2]) & all;  // window level z is shadow level z + sd[2]
}

// the leaves of level L at a node: full, and the parent is not
__device__ __forceinline__ uint64_t leafStarts(const uint64_t* pyr, uint32_t L, uint32_t node) {
  uint64_t v = pyr[levelAt(L) + node];
  if (L < 6 && v) {
    const uint32_t side = 64u >> L, x = node % side, y = node / side;
    const uint64_t p = pyr[levelAt(L + 1) + (y >> 1) * (side >> 1) + (x >> 1)];
    v &= ~(p | (p << (1u << L)));
  }
  return v;
}

__device__ __forceinline__ void storeLeaf(navgpu_c3d_leaf* out, uint32_t pos, uint32_t capacity, int32_t kx, int32_t ky, int32_t kz, uint32_t level, uint32_t cls) {
  if (pos >= capacity) return;  // (the host queues the emit only when the totals fit)
  reinterpret_cast<int4*>(out)[pos] = make_int4(kx, ky, kz, (int32_t)(level | (cls << 16)));
}

// A workgroup per (listed instance, block).  EMIT false: counts[block] = the leaves of the block.  EMIT true: the leaves, behind
// offsets[block]: the bounds plane's (DELTA), then per class; within a plane by level, coarse to fine, then key y, key x, key z.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_c3d_export(C3dDev d, C3dLayersDev ly, C3dExport e, uint32_t first) {
  __shared__ uint64_t pyr[kPyramidWords];
  __shared__ uint32_t s_wave[kScanThreads / 64];
  __shared__ uint32_t s_count[2];
  const C3dExportRec r = e.recs[first + blockIdx.y];
  if (blockIdx.x >= r.nbx * r.nby) return;  // (uniform over the workgroup, as every exit below)
  const uint32_t blk = r.first_block + blockIdx.x, tid = threadIdx.x;
  if (EMIT && !(e.counts[2 * blk] | e.counts[2 * blk + 1])) return;
  const int32_t key_x0 = (r.bx0 + (int32_t)(blockIdx.x % r.nbx)) * 64, key_y0 = (r.by0 + (int32_t)(blockIdx.x / r.nbx)) * 64;
  const int32_t wx0 = key_x0 - r.ok[0], wy0 = key_y0 - r.ok[1];  // the window column of the block's first
  // what the block publishes: everything (FULL), or the cells whose class differs from the shadow's (DELTA)
  uint64_t inside[16];
  bool any = false;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const uint32_t idx = i * 256 + tid;
    const int32_t x = wx0 + (int32_t)(idx & 63), y = wy0 + (int32_t)(idx >> 6);
    uint64_t diff = 0, present = 0;
    for (uint32_t p = 0; p < e.np; ++p) {
      const uint64_t m = masterWord(d, ly, r.instance, p, x, y);
      present |= m;
      if (e.delta) diff |= m ^ shadowWord(d, e, r, p, x, y);
    }
    if (e.delta && (x < 0 || y < 0 || x >= (int32_t)d.sx || y >= (int32_t)d.sy)) diff = 0;  // (what left the window is a forgotten box)
    inside[i] = e.delta ? diff : ~0ull;
    any = any || (e.delta ? diff : present) != 0;
  }
  if (tid < 2) s_count[tid] = 0;
  if (!__syncthreads_or(any)) {
    if (!EMIT && tid < 2) e.counts[2 * blk + tid] = 0;
    return;
  }
  uint32_t counted[2] = {0, 0};
  uint32_t at[2] = {0, 0};
  if (EMIT) {
    at[0] = e.offsets[2 * blk];
    at[1] = e.offsets[2 * blk + 1];
  }
  for (int32_t out = e.delta ? -1 : 0; out < (int32_t)e.np; ++out) {  // -1: the bounds, one binary plane
    const uint32_t channel = out < 0 ? 1u : 0u;
    __syncthreads();  // (the pyramid of the plane before has been read)
    bool some = false;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
      const uint32_t idx = i * 256 + tid;
      const uint64_t v = out < 0 ? inside[i] : masterWord(d, ly, r.instance, (uint32_t)out, wx0 + (int32_t)(idx & 63), wy0 + (int32_t)(idx >> 6)) & inside[i];
      pyr[idx] = v;
      some = some || v != 0;
    }
    if (!__syncthreads_or(some)) continue;
    uint32_t top = 0;
    for (uint32_t L = 1; L < kLevels; ++L) {
      const uint32_t side = 64u >> L, nodes = side * side, half = 1u << (L - 1);
      const uint64_t starts = alignedStarts(L, r.ok[2]);
      const uint64_t* below = pyr + levelAt(L - 1);
      bool full = false;
      for (uint32_t node = tid; node < nodes; node += 256) {
        const uint32_t x = node % side, y = node / side, c = (2 * y) * (2 * side) + 2 * x;
        const uint64_t four = below[c] & below[c + 1] & below[c + 2 * side] & below[c + 2 * side + 1];
        const uint64_t v = four & (four >> half) & starts;
        pyr[levelAt(L) + node] = v;
        full = full || v != 0;
      }
      if (!__syncthreads_or(full)) break;  // (level L stands as zeros: nothing below has a full parent)
      top = L;
    }
    for (int32_t L = (int32_t)top; L >= 0; --L) {
      const uint32_t side = 64u >> L, nodes = side * side, per = nodes >= 256 ? nodes / 256 : 1u, node0 = tid * per;
      uint32_t mine = 0;
      for (uint32_t j = 0; j < per; ++j)
        if (node0 + j < nodes) mine += (uint32_t)__popcll((ull)leafStarts(pyr, (uint32_t)L, node0 + j));
      if (!EMIT) {
        counted[channel] += mine;
        continue;
      }
      uint32_t total = 0;
      uint32_t pos = at[channel] + blockExclusive(mine, s_wave, total);
      at[channel] += total;
      if (!mine) continue;  // (past the scan's barriers)
      for (uint32_t j = 0; j < per; ++j) {
        if (node0 + j >= nodes) break;
        uint64_t v = leafStarts(pyr, (uint32_t)L, node0 + j);
        const int32_t kx = key_x0 + (int32_t)(((node0 + j) % side) << L), ky = key_y0 + (int32_t)(((node0 + j) / side) << L);
        while (v) {
          const int32_t z = __ffsll((long long)v) - 1;
          v &= v - 1;
          if (out < 0) storeLeaf(e.bounds, pos++, e.bounds_capacity, kx, ky, r.ok[2] + z, (uint32_t)L, NAVGPU_C3D_LETHAL);
          else storeLeaf(e.values, pos++, e.value_capacity, kx, ky, r.ok[2] + z, (uint32_t)L, (uint32_t)out);
        }
      }
    }
  }
  if (!EMIT) {
    if (counted[0]) atomicAdd(&s_count[0], counted[0]);
    if (counted[1]) atomicAdd(&s_count[1], counted[1]);
    __syncthreads();
    if (tid < 2) e.counts[2 * blk + tid] = s_count[tid];
  }
}

// One workgroup: offsets = the exclusive prefix of counts over the list's blocks, per channel; totals = each instance's ranges
__global__ __launch_bounds__(kScanThreads) void k_c3d_export_scan(C3dExport e) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  uint32_t carry[2] = {0, 0};
  for (uint32_t base = 0; base < e.blocks; base += kScanThreads) {
    const uint32_t i = base + threadIdx.x;
    for (uint32_t ch = 0; ch < 2; ++ch) {
      uint32_t total = 0;
      const uint32_t before = blockExclusive(i < e.blocks ? e.counts[2 * i + ch] : 0u, s_wave, total);
      if (i < e.blocks) e.offsets[2 * i + ch] = carry[ch] + before;
      carry[ch] += total;
    }
  }
  __threadfence_block();
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < e.n; k += kScanThreads)
    for (uint32_t ch = 0; ch < 2; ++ch) {
      const uint32_t begin = e.offsets[2 * e.recs[k].first_block + ch];
      const uint32_t end = k + 1 < e.n ? e.offsets[2 * e.recs[k + 1].first_block + ch] : carry[ch];
      e.totals[4 * k + 2 * ch] = begin;
      e.totals[4 * k + 2 * ch + 1] = end - begin;
    }
}

// A lane per column word of (listed instance, plane)
__global__ __launch_bounds__(256) void k_c3d_shadow_copy(C3dDev d, C3dLayersDev ly, C3dExport e, uint64_t* shadow, uint32_t first) {
  const uint32_t w = blockIdx.x * 256 + threadIdx.x, plane = blockIdx.y, inst = e.recs[first + blockIdx.z].instance;
  if (w >= d.cols) return;
  shadow[((size_t)inst * e.np + plane) * d.cols + w] = plane < 2 ? d.planes[((size_t)inst * 2 + plane) * d.cols + w] : ly.free_plane[(size_t)inst * d.cols + w];
}

// A lane per column of a leaf as the host clipped it; blockIdx.y is the leaf.  atomicOr commutes: the order of the leaves is nothing.
__global__ __launch_bounds__(256) void k_c3d_cells_raster(C3dDev d, C3dLayersDev ly, C3dCells c, uint32_t first) {
  const C3dBoxCells b = c.leaves[first + blockIdx.y];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= b.nx * b.ny) return;
  const uint32_t x = b.x0 + i % b.nx, y = b.y0 + i / b.nx;  // (inside the window: the host clipped)
  const uint32_t m = (uint32_t)b.reserved;
  atomicOr(reinterpret_cast<ull*>(c.scratch + ((size_t)m * 4 + (uint32_t)b.cls) * d.cols) + (size_t)y * d.sx + x, (ull)b.zmask);
  uint32_t* touched = c.touched + (size_t)m * ly.tw;
  const uint32_t tile = y * ly.tpr + (x >> 6);
  if (!tileBit(touched, tile)) atomicOr(touched + (tile >> 5), 1u << (tile & 31));
}

// A wave per (message, tile): CostmapLayer3D::updateCells (costmap_layer_3d.cpp:216-242).  The scratch words and the touched bit
// are cleared on the way, so the scratch is all zero again when the call has run.
__global__ __launch_bounds__(256) void k_c3d_cells_resolve(C3dDev d, C3dLayersDev ly, C3dCells c, uint32_t first) {
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= ly.tiles) return;
  const uint32_t mi = first + blockIdx.y;
  const C3dCellsMsg m = c.msgs[mi];
  uint32_t* touched = c.touched + (size_t)mi * ly.tw;
  const bool was_touched = tileBit(touched, tile);
  const int32_t y = (int32_t)(tile / ly.tpr), x0 = (int32_t)(tile % ly.tpr) * 64, x = x0 + (int32_t)lane;
  const uint32_t n_forgotten = (m.flags >> 1) & 3u;
  bool wanted = was_touched || (m.flags & 1u);
#pragma unroll
  for (uint32_t f = 0; f < 2; ++f)
    wanted = wanted || (f < n_forgotten && m.fbox[f][0] <= x0 + 63 && m.fbox[f][1] >= x0 && m.fbox[f][2] <= y && m.fbox[f][3] >= y);
  if (!wanted) return;  // (wave-uniform)
  uint64_t E = 0, kept = 0;
  if (x < (int32_t)d.sx) {
    const size_t w = (size_t)y * d.sx + (uint32_t)x;
    const uint64_t all = d.sz >= 64 ? ~0ull : (1ull << d.sz) - 1;
    uint64_t V[3] = {0, 0, 0};
    if (was_touched) {
      uint64_t* s = c.scratch + (size_t)mi * 4 * d.cols + w;
      E = s[0];
      if (E) s[0] = 0;
      for (uint32_t p = 0; p < 3; ++p) {
        V[p] = s[(size_t)(p + 1) * d.cols];
        if (V[p]) s[(size_t)(p + 1) * d.cols] = 0;
      }
    }
    if (m.flags & 1u) E = all;
#pragma unroll
    for (uint32_t f = 0; f < 2; ++f)
      if (f < n_forgotten && x >= m.fbox[f][0] && x <= m.fbox[f][1] && y >= m.fbox[f][2] && y <= m.fbox[f][3]) E |= m.fz[f];
    if (E) {
      V[kC3dN] &= ~V[kC3dL];  // the higher class wins
      V[kC3dF] &= ~(V[kC3dL] | V[kC3dN]);
      uint64_t* p = ly.set(m.instance, m.slot, m.cur, d.cols) + w;
      for (uint32_t plane = 0; plane < 3; ++plane) {
        const uint64_t old = p[(size_t)plane * d.cols], now = (old & ~E) | (V[plane] & E);
        if (now != old) p[(size_t)plane * d.cols] = now;
        kept |= now;
      }
      ly.changed[((size_t)m.instance * ly.nc + m.slot) * d.cols + w] |= E;
    }
  }
  const bool any_e = __ballot(E != 0) != 0, any_cell = __ballot(kept != 0) != 0;
  if (lane == 0) {
    if (was_touched) atomicAnd(touched + (tile >> 5), ~(1u << (tile & 31)));
    uint32_t* dirty = ly.dirty + (size_t)m.instance * ly.tw;
    if (any_e && !tileBit(dirty, tile)) atomicOr(dirty + (tile >> 5), 1u << (tile & 31));
    uint32_t* occ = ly.occOf(m.instance, m.slot, m.cur);
    if (any_cell && !tileBit(occ, tile)) atomicOr(occ + (tile >> 5), 1u << (tile & 31));  // (never cleared here: a superset costs a look)
  }
}

}  // namespace

void launch_c3d_export_count(const C3dDev& d, const C3dLayersDev& ly, const C3dExport& e, hipStream_t stream) {
  for (uint32_t first = 0; first < e.n; first += 65535u) {  // (gridDim.y)
    const uint32_t count = e.n - first < 65535u ? e.n - first : 65535u;
    hipLaunchKernelGGL(k_c3d_export<false>, dim3(e.max_blocks, count), dim3(256), 0, stream, d, ly, e, first);
  }
  hipLaunchKernelGGL(k_c3d_export_scan, dim3(1), dim3(kScanThreads), 0, stream, e);
}

void launch_c3d_export_emit(const C3dDev& d, const C3dLayersDev& ly, const C3dExport& e, hipStream_t stream) {
  for (uint32_t first = 0; first < e.n; first += 65535u) {
    const uint32_t count = e.n - first < 65535u ? e.n - first : 65535u;
    hipLaunchKernelGGL(k_c3d_export<true>, dim3(e.max_blocks, count), dim3(256), 0, stream, d, ly, e, first);
  }
}

void launch_c3d_shadow_copy(const C3dDev& d, const C3dLayersDev& ly, const C3dExport& e, uint64_t* shadow, hipStream_t stream) {
  for (uint32_t first = 0; first < e.n; first += 65535u) {  // (gridDim.z)
    const uint32_t count = e.n - first < 65535u ? e.n - first : 65535u;
    hipLaunchKernelGGL(k_c3d_shadow_copy, dim3((d.cols + 255) / 256, e.np, count), dim3(256), 0, stream, d, ly, e, shadow, first);
  }
}

void launch_c3d_cells(const C3dDev& d, const C3dLayersDev& ly, const C3dCells& c, hipStream_t stream) {
  if (c.max_columns)
    for (uint32_t first = 0; first < c.n_leaves; first += 65535u) {
      const uint32_t count = c.n_leaves - first < 65535u ? c.n_leaves - first : 65535u;
      hipLaunchKernelGGL(k_c3d_cells_raster, dim3((c.max_columns + 255) / 256, count), dim3(256), 0, stream, d, ly, c, first);
    }
  for (uint32_t first = 0; first < c.n_msgs; first += 65535u) {
    const uint32_t count = c.n_msgs - first < 65535u ? c.n_msgs - first : 65535u;
    hipLaunchKernelGGL(k_c3d_cells_resolve, dim3((ly.tiles + 3) / 4, count), dim3(256), 0, stream, d, ly, c, first);
  }
}

}  // namespace navgpu
