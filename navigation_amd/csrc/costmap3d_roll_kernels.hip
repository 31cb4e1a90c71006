// Rolling 3-D maps and resetBoundingBox on the bit volumes of a navgpu_costmap3d handle (include/navgpu_costmap3d_rolling.h).
// A roll moves every object of an instance - a plane of column words, or the 2-D layer's bytes - in place: dst(x, y) =
// src(x + dx, y + dy), or empty off the window.  It is two passes, each right whatever order its workgroups run in:
//   k_c3d_roll_y  a lane owns one column of one object and walks its rows in the direction of dy; it has loaded a row |dy| steps
//                 before it stores to it, and no other lane touches its column;
//   k_c3d_roll_x  a workgroup owns one row of one object: it loads a chunk of the row, crosses a barrier and stores the chunk
//                 shifted; chunks go in the direction of dx, so no chunk reads what an earlier one wrote.  No other workgroup
//                 touches the row.
// k_c3d_roll_bits then rebuilds the tile bitmaps k_c3d_layer_swap and k_c3d_combine skip tiles by, from the data itself.
// A tile is 64 consecutive column words of a row: a wave.  Everything is integers and bits.
#include "navgpu_costmap3d.h"

namespace navgpu {
namespace {

__device__ __forceinline__ bool tileBit(const uint32_t* map, uint32_t tile) { return (map[tile >> 5] >> (tile & 31)) & 1u; }

// The objects of an instance: the master's LETHAL and NONLETHAL planes; on a layered handle also its FREE plane, every costmap
// layer's current planes and changed plane, and the 2-D layer's bytes (the last object).
__device__ __forceinline__ uint32_t rollObjects(const C3dLayersDev& ly, int32_t layered) { return layered ? 4u + 4u * ly.nc : 2u; }
__device__ __forceinline__ uint64_t* rollPlane(const C3dDev& d, const C3dLayersDev& ly, const C3dRollRec& r, uint32_t obj) {
  if (obj < 2) return d.planes + ((size_t)r.instance * 2 + obj) * d.cols;
  if (obj == 2) return ly.free_plane + (size_t)r.instance * d.cols;
  const uint32_t slot = (obj - 3) >> 2, p = (obj - 3) & 3;
  if (p == 3) return ly.changed + ((size_t)r.instance * ly.nc + slot) * d.cols;
  return ly.set(r.instance, slot, (r.cur_bits >> slot) & 1u, d.cols) + (size_t)p * d.cols;
}

constexpr int kRollAhead = 8;  // rows a lane loads before it stores them: a walk is not one round trip per row

// one column of one object: rows in the direction of dy, kRollAhead at a time.  A group's loads lie |dy| rows ahead of its own
// stores and of every earlier group's, so nothing is read after it has been overwritten.
template <class T>
__device__ __forceinline__ void rollColumn(T* column, uint32_t sx, uint32_t sy, int32_t dy, T empty) {
  const int64_t step = dy > 0 ? 1 : -1;
  int64_t y = dy > 0 ? 0 : (int64_t)sy - 1;
  for (uint32_t done = 0; done < sy; done += kRollAhead, y += kRollAhead * step) {
    T v[kRollAhead];
#pragma unroll
    for (int k = 0; k < kRollAhead; ++k) {
      const int64_t src = y + k * step + dy;
      v[k] = (done + k < sy && src >= 0 && src < (int64_t)sy) ? column[(size_t)src * sx] : empty;
    }
#pragma unroll
    for (int k = 0; k < kRollAhead; ++k)
      if (done + k < sy) column[(size_t)(y + k * step) * sx] = v[k];
  }
}

// A wave per (moved instance, object, stripe of 64 columns), a lane per column
__global__ __launch_bounds__(256) void k_c3d_roll_y(C3dDev d, C3dLayersDev ly, int32_t layered, const C3dRollRec* recs) {
  const C3dRollRec r = recs[blockIdx.z];
  if (r.dy == 0 || (r.cur_bits & kC3dRollEmpty)) return;
  const uint32_t x = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63), obj = blockIdx.y;
  if (x >= d.sx) return;
  if (layered && obj + 1 == rollObjects(ly, layered))
    rollColumn<uint8_t>(ly.layer2d + (size_t)r.instance * d.cols + x, d.sx, d.sy, r.dy, 255);  // NO_INFORMATION
  else
    rollColumn<uint64_t>(rollPlane(d, ly, r, obj) + x, d.sx, d.sy, r.dy, 0);
}

// one row of one object by a workgroup: chunks of kC3dRollRow columns in the direction of dx, loaded, a barrier, stored shifted.
// A chunk's loads lie |dx| columns ahead of every store so far; its own stores come behind the barrier.
template <class T>
__device__ __forceinline__ void rollRow(T* row, uint32_t sx, int32_t dx, bool everything_leaves, T empty) {
  if (everything_leaves) {  // a fill, not a walk
    for (uint32_t x = threadIdx.x; x < sx; x += 256) row[x] = empty;
    return;
  }
  const uint32_t chunks = (sx + kC3dRollRow - 1) / kC3dRollRow;
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint32_t x0 = (dx > 0 ? c : chunks - 1 - c) * kC3dRollRow + threadIdx.x;
    T v[kC3dRollRow / 256];
#pragma unroll
    for (uint32_t k = 0; k < kC3dRollRow / 256; ++k) {
      const int64_t src = (int64_t)x0 + 256 * k + dx;
      v[k] = (x0 + 256 * k < sx && src >= 0 && src < (int64_t)sx) ? row[src] : empty;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kC3dRollRow / 256; ++k)
      if (x0 + 256 * k < sx) row[x0 + 256 * k] = v[k];
  }
}

// A workgroup per (moved instance, object, row)
__global__ __launch_bounds__(256) void k_c3d_roll_x(C3dDev d, C3dLayersDev ly, int32_t layered, const C3dRollRec* recs) {
  const C3dRollRec r = recs[blockIdx.z];
  const bool everything_leaves = (r.cur_bits & kC3dRollEmpty) != 0;
  if (r.dx == 0 && !everything_leaves) return;  // (uniform over the workgroup, as everything below but the lanes' columns)
  const uint32_t y = blockIdx.x, obj = blockIdx.y;
  if (layered && obj + 1 == rollObjects(ly, layered))
    rollRow<uint8_t>(ly.layer2d + (size_t)r.instance * d.cols + (size_t)y * d.sx, d.sx, r.dx, everything_leaves, 255);
  else
    rollRow<uint64_t>(rollPlane(d, ly, r, obj) + (size_t)y * d.sx, d.sx, r.dx, everything_leaves, 0);
}

// A lane per moved instance: the device's copy of the origin follows in stream order
__global__ void k_c3d_roll_origins(C3dDev d, const C3dRollRec* recs, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  d.origins[3 * (size_t)recs[k].instance] = recs[k].ox;
  d.origins[3 * (size_t)recs[k].instance + 1] = recs[k].oy;
}

// A wave per (moved instance, bitmap, tile), after the shift.  Bitmap s < nc: the occupancy of slot s' current set, set exactly for
// the tiles that hold a cell (the next scratch set is empty and its bits are clear: nothing moved there).  Bitmap nc: the instance's
// dirty bits, set exactly for the tiles with a changed bit.  Only this wave writes its tile's bit in this launch.
__global__ __launch_bounds__(256) void k_c3d_roll_bits(C3dDev d, C3dLayersDev ly, const C3dRollRec* recs) {
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile >= ly.tiles) return;
  const C3dRollRec r = recs[blockIdx.z];
  const uint32_t map_index = blockIdx.y;
  const uint32_t y = tile / ly.tpr, x = (tile % ly.tpr) * 64 + lane;
  uint64_t v = 0;
  if (x < d.sx) {
    const size_t w = (size_t)y * d.sx + x;
    if (map_index < ly.nc) {
      const uint64_t* p = ly.set(r.instance, map_index, (r.cur_bits >> map_index) & 1u, d.cols) + w;
      v = p[0] | p[d.cols] | p[2 * (size_t)d.cols];
    } else {
      for (uint32_t s = 0; s < ly.nc; ++s) v |= ly.changed[((size_t)r.instance * ly.nc + s) * d.cols + w];
    }
  }
  const bool any = __ballot(v != 0) != 0;
  if (lane == 0) {
    uint32_t* map = map_index < ly.nc ? ly.occOf(r.instance, map_index, (r.cur_bits >> map_index) & 1u) : ly.dirty + (size_t)r.instance * ly.tw;
    const bool is_set = tileBit(map, tile);
    if (any && !is_set) atomicOr(map + (tile >> 5), 1u << (tile & 31));
    if (!any && is_set) atomicAnd(map + (tile >> 5), ~(1u << (tile & 31)));
  }
}

// A wave per (listed instance, named POINT_CLOUD layer, tile meeting the clipped box): CostmapLayer3D::resetBoundingBox
// (costmap_layer_3d.cpp:149-191).  The occupancy bit may stay set: a superset costs a look, a stale clear bit would lose data.
__global__ __launch_bounds__(256) void k_c3d_reset_box(C3dDev d, C3dLayersDev ly, const C3dResetRec* recs, C3dResetSlots slots) {
  const C3dResetRec r = recs[blockIdx.z];
  const uint32_t tx0 = r.x0 >> 6, ntx = (r.x1 >> 6) - tx0 + 1, nty = r.y1 - r.y0 + 1;
  const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= ntx * nty) return;
  const uint32_t y = r.y0 + t / ntx, tx = tx0 + t % ntx, x = tx * 64 + lane;
  const uint32_t slot = slots.slot[blockIdx.y];
  uint64_t removed = 0;
  if (x >= r.x0 && x <= r.x1) {  // (x1 < size_x)
    const size_t w = (size_t)y * d.sx + x;
    uint64_t* p = ly.set(r.instance, slot, (r.cur_bits >> slot) & 1u, d.cols) + w;
    for (uint32_t plane = 0; plane < 3; ++plane) {
      const uint64_t word = p[(size_t)plane * d.cols], gone = word & r.zmask;
      if (gone) p[(size_t)plane * d.cols] = word & ~r.zmask;
      removed |= gone;
    }
    if (removed) ly.changed[((size_t)r.instance * ly.nc + slot) * d.cols + w] |= removed;
  }
  const bool any = __ballot(removed != 0) != 0;
  if (lane == 0 && any) {
    uint32_t* dirty = ly.dirty + (size_t)r.instance * ly.tw;
    const uint32_t tile = y * ly.tpr + tx;
    if (!tileBit(dirty, tile)) atomicOr(dirty + (tile >> 5), 1u << (tile & 31));
  }
}

}  // namespace

void launch_c3d_roll(const C3dDev& d, const C3dLayersDev& ly, int32_t layered, const C3dRollRec* recs, uint32_t n, bool any_y, bool any_x,
                     hipStream_t stream) {
  const uint32_t objects = layered ? 4u + 4u * ly.nc : 2u;
  hipLaunchKernelGGL(k_c3d_roll_origins, dim3((n + 255) / 256), dim3(256), 0, stream, d, recs, n);
  for (uint32_t first = 0; first < n; first += 65535u) {  // (gridDim.z)
    const uint32_t count = n - first < 65535u ? n - first : 65535u;
    if (any_y) hipLaunchKernelGGL(k_c3d_roll_y, dim3(((d.sx + 63) / 64 + 3) / 4, objects, count), dim3(256), 0, stream, d, ly, layered, recs + first);
    if (any_x) hipLaunchKernelGGL(k_c3d_roll_x, dim3(d.sy, objects, count), dim3(256), 0, stream, d, ly, layered, recs + first);
    if (layered) hipLaunchKernelGGL(k_c3d_roll_bits, dim3((ly.tiles + 3) / 4, ly.nc + 1, count), dim3(256), 0, stream, d, ly, recs + first);
  }
}

void launch_c3d_reset_box(const C3dDev& d, const C3dLayersDev& ly, const C3dResetRec* recs, uint32_t n, uint32_t max_tiles, const C3dResetSlots& slots,
                          hipStream_t stream) {
  if (!slots.n || !max_tiles) return;
  for (uint32_t first = 0; first < n; first += 65535u) {
    const uint32_t count = n - first < 65535u ? n - first : 65535u;
    hipLaunchKernelGGL(k_c3d_reset_box, dim3((max_tiles + 3) / 4, slots.n, count), dim3(256), 0, stream, d, ly, recs + first, slots);
  }
}

}  // namespace navgpu
