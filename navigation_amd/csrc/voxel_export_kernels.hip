// HIP kernels (gfx950) behind navgpu_voxel_points and navgpu_voxel_clearing_endpoints: the voxel layer's debug outputs as
// order-preserving stream compactions of what is resident.
//   voxel points      : costmap_2d_cloud.cpp:85-122 / costmap_2d_markers.cpp:84-108 - every voxel of one status in the loop order
//                       y, x, z.  A robot's columns in row-major order ARE the (y, x) order and a column's voxels are the set
//                       bits of a 16-bit mask in ascending z (marked = hi & lo, unknown = hi ^ lo), so no lane loops over z to
//                       classify: popc counts, a bit scan emits.
//   clearing endpoints: voxel_layer.cpp:286-381 - the clipped ray end of every point of every staged clearing observation that
//                       passes worldToMap3DFloat, in staging then cloud order; the predicate and the end are voxelRayBegin /
//                       voxelRayEnd of navgpu_device.h, which k_obstacle<true>'s clearRaysVoxel walks its rays to.
// Both are three launches over fixed-size chunks of the input:
//   (a) count : a workgroup per (chunk, robot) - per (chunk of points, observation, robot) for the endpoints - writes ONE total
//   (b) scan  : a workgroup per robot scans its totals exclusively, in tiles of 256 with a carry, and writes the robot's count
//               (and the per-observation counts)
//   (c) emit  : as (a), each lane recomputes its offset inside the chunk - shuffles inside the wave, the waves' totals through
//               LDS - and writes at base + offset while that is below the capacity
// No atomic decides a position: the output is the same bytes from run to run.  Compiled with -ffp-contract=off.
#include "block_scan.h"
#include "navgpu_device.h"

namespace navgpu {

static_assert(kVxThreads == kScanThreads, "blockExclusive (block_scan.h) scans a workgroup of kScanThreads lanes");

// ------------------------------------------------------------------------------------------------ voxel points
// the z bits of a column whose VoxelGrid::getVoxel (voxel_grid.h:183-206) equals the status asked for
__device__ __forceinline__ uint32_t statusBits(uint32_t col, uint32_t zmask, bool marked) {
  const uint32_t hi = col >> 16, lo = col & 0xFFFFu;
  return (marked ? (hi & lo) : (hi ^ lo)) & zmask;
}

// the lane's kVxPerLane masks; columns past the grid (cells .. cells_padded) count as empty
__device__ __forceinline__ void laneColumns(const CostmapDev& cm, uint32_t inst, uint32_t c0, uint32_t zmask, bool marked, uint32_t bits[kVxPerLane]) {
#pragma unroll
  for (uint32_t j = 0; j < kVxPerLane; ++j) bits[j] = 0;
  if (c0 >= cm.cells) return;
  // c0 is a multiple of 4 below cells <= cells_padded, itself a multiple of 64: the 16 bytes are the robot's own, and aligned
  const uint4 q = *reinterpret_cast<const uint4*>(cm.voxel + (size_t)inst * cm.cells_padded + c0);
  const uint32_t w[kVxPerLane] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (uint32_t j = 0; j < kVxPerLane; ++j) bits[j] = (c0 + j < cm.cells) ? statusBits(w[j], zmask, marked) : 0u;
}

__global__ __launch_bounds__(kVxThreads) void k_voxel_count(CostmapDev cm, VoxelExportDev v, uint32_t first, uint32_t zmask) {
  __shared__ uint32_t s_wave[kVxThreads / 64];
  const uint32_t k = blockIdx.y, inst = first + k;
  uint32_t bits[kVxPerLane];
  laneColumns(cm, inst, blockIdx.x * kVxChunk + threadIdx.x * kVxPerLane, zmask, v.status == NAVGPU_VOXEL_MARKED, bits);
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kVxPerLane; ++j) mine += __popc(bits[j]);
  uint32_t total;
  blockExclusive(mine, s_wave, total);
  if (threadIdx.x == 0) v.totals[(size_t)k * v.stride + blockIdx.x] = total;
}

// (b) for both: totals[k][0 .. n_totals) become their exclusive prefix, counts[k] their sum.  With seg_counts: the totals are
// n_seg runs of seg_len (an observation's chunks) and seg_counts[k][s] is the sum of run s.
__global__ __launch_bounds__(kVxThreads) void k_export_scan(VoxelExportDev v, uint32_t n_totals, uint32_t n_seg, uint32_t seg_len) {
  __shared__ uint32_t s_wave[kVxThreads / 64];
  const uint32_t k = blockIdx.x;
  uint32_t* tot = v.totals + (size_t)k * v.stride;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_totals; base += kVxThreads) {  // (uniform: every lane runs every tile)
    const uint32_t i = base + threadIdx.x;
    const uint32_t mine = i < n_totals ? tot[i] : 0u;
    uint32_t tile;
    const uint32_t ex = blockExclusive(mine, s_wave, tile);
    if (i < n_totals) tot[i] = carry + ex;
    carry += tile;
  }
  if (threadIdx.x == 0) v.counts[k] = carry;
  if (n_seg) {
    __syncthreads();  // the prefixes this workgroup wrote
    for (uint32_t s = threadIdx.x; s < n_seg; s += kVxThreads)
      v.obs_counts[(size_t)k * n_seg + s] = (s + 1 < n_seg ? tot[(size_t)(s + 1) * seg_len] : carry) - tot[(size_t)s * seg_len];
  }
}

// mapToWorld3D (costmap_2d_cloud.cpp:36-42) in double; T = float narrows as the assignment to a Point32 does
template <class T>
__global__ __launch_bounds__(kVxThreads) void k_voxel_emit(CostmapDev cm, VoxelExportDev v, uint32_t first, uint32_t zmask) {
  __shared__ uint32_t s_wave[kVxThreads / 64];
  const uint32_t k = blockIdx.y, inst = first + k;
  const uint32_t c0 = blockIdx.x * kVxChunk + threadIdx.x * kVxPerLane;
  uint32_t bits[kVxPerLane];
  laneColumns(cm, inst, c0, zmask, v.status == NAVGPU_VOXEL_MARKED, bits);
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kVxPerLane; ++j) mine += __popc(bits[j]);
  uint32_t total;
  uint32_t at = v.totals[(size_t)k * v.stride + blockIdx.x] + blockExclusive(mine, s_wave, total);
  if (mine == 0 || at >= v.capacity) return;
  const double ox = cm.origin[2 * inst], oy = cm.origin[2 * inst + 1];
  T* out = static_cast<T*>(v.xyz) + (size_t)k * v.capacity * 3;
#pragma unroll
  for (uint32_t j = 0; j < kVxPerLane; ++j) {
    uint32_t b = bits[j];
    if (!b) continue;
    const uint32_t c = c0 + j, my = c / cm.nx, mx = c - my * cm.nx;
    const double wx = ox + (mx + 0.5) * cm.res, wy = oy + (my + 0.5) * cm.res;
    while (b && at < v.capacity) {
      const uint32_t mz = __ffs(b) - 1;
      b &= b - 1;
      const double wz = cm.origin_z + (mz + 0.5) * cm.z_resolution;
      out[(size_t)at * 3] = (T)wx;
      out[(size_t)at * 3 + 1] = (T)wy;
      out[(size_t)at * 3 + 2] = (T)wz;
      ++at;
    }
  }
}

void launch_voxel_points_count(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s) {
  const uint32_t chunks = voxel_export_chunks(cm.cells);
  const uint32_t zmask = (uint32_t)((1ull << (cm.z_voxels > 16 ? 16 : cm.z_voxels)) - 1);
  hipLaunchKernelGGL(k_voxel_count, dim3(chunks, count), dim3(kVxThreads), 0, s, cm, v, first, zmask);
  hipLaunchKernelGGL(k_export_scan, dim3(count), dim3(kVxThreads), 0, s, v, chunks, 0u, 0u);
}

void launch_voxel_points_emit(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s) {
  const uint32_t chunks = voxel_export_chunks(cm.cells);
  const uint32_t zmask = (uint32_t)((1ull << (cm.z_voxels > 16 ? 16 : cm.z_voxels)) - 1);
  if (v.as_double)
    hipLaunchKernelGGL(k_voxel_emit<double>, dim3(chunks, count), dim3(kVxThreads), 0, s, cm, v, first, zmask);
  else
    hipLaunchKernelGGL(k_voxel_emit<float>, dim3(chunks, count), dim3(kVxThreads), 0, s, cm, v, first, zmask);
}

// ------------------------------------------------------------------------------------------------ clearing endpoints
// the lane's point of (robot, observation, chunk): kept or not, and its clipped ray end
__device__ __forceinline__ bool clearPoint(const CostmapDev& cm, uint32_t inst, double& wpx, double& wpy, double& wpz) {
  const uint32_t o = blockIdx.y;
  if (o >= cm.obs_count[inst]) return false;
  const ObsCsr obs = cm.obs[(size_t)inst * cm.max_obs + o];
  const uint32_t p = blockIdx.x * kClearChunk + threadIdx.x;
  if (!(obs.flags & NAVGPU_OBS_CLEARING) || p >= obs.n_points) return false;
  const Geom g{cm.origin[2 * inst], cm.origin[2 * inst + 1], cm.res, cm.nx, cm.ny};
  const uint32_t size_z = (uint32_t)(cm.z_voxels > 16 ? 16 : cm.z_voxels);
  VoxelRay ray;
  if (!voxelRayBegin(g, cm, size_z, obs, ray)) return false;
  const float* pt = cm.points + ((size_t)inst * cm.max_points + obs.first_point + p) * 3;
  double px, py, pz;
  return voxelRayEnd(g, cm, size_z, ray, pt, wpx, wpy, wpz, px, py, pz);
}

__global__ __launch_bounds__(kVxThreads) void k_clear_count(CostmapDev cm, VoxelExportDev v, uint32_t first) {
  __shared__ uint32_t s_wave[kVxThreads / 64];
  const uint32_t k = blockIdx.z, inst = first + k;
  double wpx, wpy, wpz;
  const bool keep = clearPoint(cm, inst, wpx, wpy, wpz);
  uint32_t total;
  blockExclusive(keep ? 1u : 0u, s_wave, total);
  if (threadIdx.x == 0) v.totals[(size_t)k * v.stride + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(kVxThreads) void k_clear_emit(CostmapDev cm, VoxelExportDev v, uint32_t first) {
  __shared__ uint32_t s_wave[kVxThreads / 64];
  const uint32_t k = blockIdx.z, inst = first + k;
  double wpx = 0, wpy = 0, wpz = 0;
  const bool keep = clearPoint(cm, inst, wpx, wpy, wpz);
  uint32_t total;
  const uint32_t at = v.totals[(size_t)k * v.stride + (size_t)blockIdx.y * gridDim.x + blockIdx.x] + blockExclusive(keep ? 1u : 0u, s_wave, total);
  if (!keep || at >= v.capacity) return;
  float* out = static_cast<float*>(v.xyz) + ((size_t)k * v.capacity + at) * 3;
  out[0] = (float)wpx;  // geometry_msgs::Point32 (voxel_layer.cpp:366-370)
  out[1] = (float)wpy;
  out[2] = (float)wpz;
}

void launch_clear_endpoints_count(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s) {
  const uint32_t chunks = clear_export_chunks(cm.max_points);
  hipLaunchKernelGGL(k_clear_count, dim3(chunks, cm.max_obs, count), dim3(kVxThreads), 0, s, cm, v, first);
  hipLaunchKernelGGL(k_export_scan, dim3(count), dim3(kVxThreads), 0, s, v, chunks * cm.max_obs, cm.max_obs, chunks);
}

void launch_clear_endpoints_emit(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s) {
  hipLaunchKernelGGL(k_clear_emit, dim3(clear_export_chunks(cm.max_points), cm.max_obs, count), dim3(kVxThreads), 0, s, cm, v, first);
}

}  // namespace navgpu
