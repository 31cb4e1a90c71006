// C-ABI host side of the voxel layer's debug outputs (include/navgpu.h):
//   navgpu_voxel_points              what costmap_2d_cloud / costmap_2d_markers make of the voxel_grid message
//   navgpu_voxel_clearing_endpoints  the clearing_endpoints cloud of VoxelLayer::raytraceFreespace
// Both are the count / scan / emit launches of voxel_export_kernels.hip on the fleet's stream.  The host reads the counts
// between (b) and (c): the device buffer of the points is sized by what is there (and by the caller's capacity), not by
// the grid, and a robot's points are copied out in its true number.
#include "navgpu_fleet.h"

namespace {

// room for `bytes` of points on the device.  All-or-nothing: the fleet keeps its buffer when the allocation fails.
int reservePoints(navgpu_fleet* f, size_t bytes) {
  navgpu_fleet::VoxelExport& vx = f->vx;
  if (bytes <= vx.xyz_bytes) return NAVGPU_OK;
  size_t cap = std::max<size_t>(vx.xyz_bytes, (size_t)1 << 16);
  while (cap < bytes) cap *= 2;
  uint8_t* q = nullptr;
  int rc = f->alloc(&q, cap);
  if (rc) return rc;
  HIP_TRY(waitStream(f->stream));  // (the fresh buffer's memset; nothing queued reads the old one)
  f->release(vx.d_xyz);
  vx.d_xyz = q;
  vx.xyz_bytes = cap;
  return NAVGPU_OK;
}

// (c) and the copies out: robot k's min(count, capacity) points go to the caller's block k.  h_counts holds the counts.
template <class Emit>
int emitPoints(navgpu_fleet* f, VoxelExportDev& v, uint32_t count, uint32_t capacity, size_t elem, void* xyz, Emit emit) {
  const uint32_t* h_counts = f->vx.h_counts;
  uint32_t most = 0;
  for (uint32_t k = 0; k < count; ++k) most = std::max(most, h_counts[k]);
  const uint32_t dev_cap = std::min(most, capacity);
  if (!xyz || dev_cap == 0) return NAVGPU_OK;
  int rc = reservePoints(f, (size_t)count * dev_cap * 3 * elem);
  if (rc) return rc;
  v.xyz = f->vx.d_xyz;
  v.capacity = dev_cap;
  PROFILED(f, NAVGPU_K_VOXEL_EXPORT, emit());
  if ((rc = checkLaunch())) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t here = std::min(h_counts[k], capacity);
    if (here)
      HIP_TRY(hipMemcpyAsync((char*)xyz + (size_t)k * capacity * 3 * elem, (const char*)v.xyz + (size_t)k * dev_cap * 3 * elem, (size_t)here * 3 * elem,
                             hipMemcpyDeviceToHost, f->stream));
  }
  HIP_TRY(waitStream(f->stream));
  return NAVGPU_OK;
}

bool exportArgsOk(const navgpu_fleet* f, uint32_t first, uint32_t count, uint32_t capacity, const void* xyz, const uint32_t* counts) {
  return f && counts && f->rangeOk(first, count) && count <= 65535 && (f->cm.layers & NAVGPU_LAYER_VOXEL) && f->cm.voxel && (xyz || capacity == 0);
}

}  // namespace

extern "C" {

int navgpu_voxel_points(navgpu_fleet* f, uint32_t first, uint32_t count, int status, int as_double, uint32_t capacity, void* xyz, uint32_t* counts) {
  if (!exportArgsOk(f, first, count, capacity, xyz, counts) || (status != NAVGPU_VOXEL_UNKNOWN && status != NAVGPU_VOXEL_MARKED))
    return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (f->desc.rolling_window && f->shift_pending) return NAVGPU_ERR_STATE;  // the grids lag the origins until the update
  navgpu_fleet::VoxelExport& vx = f->vx;
  VoxelExportDev v{};
  v.totals = vx.d_totals;
  v.stride = vx.stride;
  v.counts = vx.d_counts;
  v.status = status;
  v.as_double = as_double != 0;
  PROFILED(f, NAVGPU_K_VOXEL_EXPORT, launch_voxel_points_count(f->cm, v, first, count, f->stream));
  int rc = checkLaunch();
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(vx.h_counts, vx.d_counts, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  rc = emitPoints(f, v, count, capacity, as_double ? sizeof(double) : sizeof(float), xyz,
                  [&] { launch_voxel_points_emit(f->cm, v, first, count, f->stream); });
  if (rc) return rc;
  memcpy(counts, vx.h_counts, sizeof(uint32_t) * count);
  return NAVGPU_OK;
}

int navgpu_voxel_clearing_endpoints(navgpu_fleet* f, uint32_t first, uint32_t count, uint32_t capacity, float* xyz, uint32_t* obs_counts,
                                    uint32_t* counts) {
  if (!exportArgsOk(f, first, count, capacity, xyz, counts) || !obs_counts || f->cm.max_obs > 65535) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (f->desc.rolling_window && f->shift_pending) return NAVGPU_ERR_STATE;
  for (uint32_t i = first; i < first + count; ++i)
    if (!f->obs_consumed[i]) return NAVGPU_ERR_STATE;  // the reference clips with the origin AFTER updateOrigin (voxel_layer.cpp:119-120)
  navgpu_fleet::VoxelExport& vx = f->vx;
  const uint32_t max_obs = f->cm.max_obs;
  if (!f->cm.obs_enabled) {  // VoxelLayer::updateBounds returns before raytraceFreespace (:121-122)
    memset(counts, 0, sizeof(uint32_t) * count);
    memset(obs_counts, 0, sizeof(uint32_t) * (size_t)count * max_obs);
    return NAVGPU_OK;
  }
  VoxelExportDev v{};
  v.totals = vx.d_totals;
  v.stride = vx.stride;
  v.counts = vx.d_counts;
  v.obs_counts = vx.d_obs_counts;
  PROFILED(f, NAVGPU_K_VOXEL_EXPORT, launch_clear_endpoints_count(f->cm, v, first, count, f->stream));
  int rc = checkLaunch();
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(vx.h_counts, vx.d_counts, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(hipMemcpyAsync(vx.h_obs_counts, vx.d_obs_counts, sizeof(uint32_t) * (size_t)count * max_obs, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  rc = emitPoints(f, v, count, capacity, sizeof(float), xyz, [&] { launch_clear_endpoints_emit(f->cm, v, first, count, f->stream); });
  if (rc) return rc;
  memcpy(counts, vx.h_counts, sizeof(uint32_t) * count);
  memcpy(obs_counts, vx.h_obs_counts, sizeof(uint32_t) * (size_t)count * max_obs);
  return NAVGPU_OK;
}

}  // extern "C"
