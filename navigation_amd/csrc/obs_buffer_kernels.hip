// HIP kernels (gfx950) behind navgpu_obsbuf_*: costmap_2d::ObservationBuffer's point work on device-resident rings.
//   k_obs_ingest      : bufferCloud (observation_buffer.cpp:154-179) for the clouds of one call - projection of a scan's beams,
//                       the cloud transform, the height filter, and an order-preserving compaction into the cloud's ring slot.
//                       One workgroup per cloud walks it in tiles of 256 with a carry; the last tile writes the slot's count.
//   k_obs_gather      : what getObservations (:198-209) copies out, straight into the arrays k_obstacle reads: one workgroup
//                       per robot completes the descriptors the host staged (first_point, n_points from the slots' counts) and
//                       copies the slots' points into the robot's block of cm.points.
//   k_obs_retransform : setGlobalFrame's cloud transform (:96) on the kept slots, in place, one lane per point.
// No atomic decides a position: the rings hold the same bytes from run to run.  Compiled with -ffp-contract=off: the fp32
// transform below is unfused, in the order include/navgpu.h states.
#include "block_scan.h"
#include "navgpu_device.h"

namespace navgpu {

// pcl::transformPointCloud's per-point arithmetic as navgpu.h restates it: fp32, left to right
__device__ __forceinline__ void cloudTransform(const float* m, float x, float y, float z, float& tx, float& ty, float& tz) {
  tx = ((m[0] * x + m[1] * y) + m[2] * z) + m[9];
  ty = ((m[3] * x + m[4] * y) + m[5] * z) + m[10];
  tz = ((m[6] * x + m[7] * y) + m[8] * z) + m[11];
}

__global__ __launch_bounds__(kScanThreads) void k_obs_ingest(ObsBufDev ob, const ObsIngestCloud* __restrict__ clouds, const float* __restrict__ points,
                                                             const float* __restrict__ ranges) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  __shared__ ObsIngestCloud s_c;
  if (threadIdx.x < sizeof(ObsIngestCloud) / 4)
    reinterpret_cast<uint32_t*>(&s_c)[threadIdx.x] = reinterpret_cast<const uint32_t*>(clouds + blockIdx.x)[threadIdx.x];
  __syncthreads();
  const ObsIngestCloud& c = s_c;
  float* out = ob.ring + (size_t)c.slot * ob.max_cloud_points * 3;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < c.n; base += kScanThreads) {  // (uniform: every lane runs every tile)
    const uint32_t i = base + threadIdx.x;
    bool keep = i < c.n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (keep) {
      if (c.kind == NAVGPU_CLOUD_SCAN) {
        float r = ranges[c.first + i];
        if (c.inf_is_valid && !isfinite(r) && r > 0.f) r = c.range_max - 0.0001f;  // obstacle_layer.cpp:281-289
        keep = r >= c.range_min && r < c.range_max;
        if (keep) {  // projectLaser: double sincos of the beam's angle, narrowed once per coordinate
          const double a = (double)c.angle_min + (double)i * (double)c.angle_increment;
          double sn, cs;
          sincos(a, &sn, &cs);
          x = (float)((double)r * cs);
          y = (float)((double)r * sn);
        }
      } else {
        const float* p = points + (size_t)(c.first + i) * 3;
        x = p[0];
        y = p[1];
        z = p[2];
      }
    }
    float tx, ty, tz;
    cloudTransform(c.m, x, y, z, tx, ty, tz);
    keep = keep && (double)tz <= c.max_h && (double)tz >= c.min_h;  // observation_buffer.cpp:169-170 (NaN drops)
    uint32_t tile;
    const uint32_t at = carry + blockExclusive(keep ? 1u : 0u, s_wave, tile);
    if (keep) {  // at < c.n <= max_cloud_points: inside the slot
      out[(size_t)at * 3] = tx;
      out[(size_t)at * 3 + 1] = ty;
      out[(size_t)at * 3 + 2] = tz;
    }
    carry += tile;
  }
  if (threadIdx.x == 0) ob.counts[c.slot] = carry;
}

// The host staged the robot's descriptors (cm.obs, cm.obs_count) with the ring slot of each in `pad`.
template <class Robots>
__global__ __launch_bounds__(kScanThreads) void k_obs_gather(ObsBufDev ob, CostmapDev cm, Robots robots) {
  const uint32_t inst = robots(blockIdx.x);
  ObsCsr* obs = cm.obs + (size_t)inst * cm.max_obs;
  const uint32_t n_obs = min(cm.obs_count[inst], cm.max_obs);
  const size_t slot0 = (size_t)inst * ob.slots_per_robot;
  if (threadIdx.x == 0) {  // a handful of entries: exclusive offsets of the slots' counts
    uint32_t off = 0;
    for (uint32_t k = 0; k < n_obs; ++k) {
      const uint32_t n = min(ob.counts[slot0 + obs[k].pad], cm.max_points - off);  // (the host's upper-bound check keeps the sum inside)
      obs[k].first_point = off;
      obs[k].n_points = n;
      off += n;
    }
  }
  __syncthreads();
  float* dst = cm.points + (size_t)inst * cm.max_points * 3;
  for (uint32_t k = 0; k < n_obs; ++k) {
    const float* src = ob.ring + (slot0 + obs[k].pad) * ob.max_cloud_points * 3;
    float* d = dst + (size_t)obs[k].first_point * 3;
    const uint32_t words = obs[k].n_points * 3;
    for (uint32_t j = threadIdx.x; j < words; j += kScanThreads) d[j] = src[j];
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < n_obs; k += kScanThreads) obs[k].pad = 0;
}

__global__ __launch_bounds__(kScanThreads) void k_obs_retransform(ObsBufDev ob, const ObsRetransform* __restrict__ items) {
  const ObsRetransform& it = items[blockIdx.y];
  const uint32_t i = blockIdx.x * kScanThreads + threadIdx.x;
  if (i >= ob.counts[it.slot]) return;
  float* p = ob.ring + ((size_t)it.slot * ob.max_cloud_points + i) * 3;
  float tx, ty, tz;
  cloudTransform(it.m, p[0], p[1], p[2], tx, ty, tz);
  p[0] = tx;
  p[1] = ty;
  p[2] = tz;
}

void launch_obs_ingest(const ObsBufDev& ob, const ObsIngestCloud* clouds, uint32_t n_clouds, const float* points, const float* ranges, hipStream_t s) {
  hipLaunchKernelGGL(k_obs_ingest, dim3(n_clouds), dim3(kScanThreads), 0, s, ob, clouds, points, ranges);
}
void launch_obs_gather(const ObsBufDev& ob, const CostmapDev& cm, uint32_t first, uint32_t count, hipStream_t s) {
  hipLaunchKernelGGL(k_obs_gather<RobotRange>, dim3(count), dim3(kScanThreads), 0, s, ob, cm, RobotRange{first});
}
void launch_obs_gather(const ObsBufDev& ob, const CostmapDev& cm, RobotList robots, uint32_t count, hipStream_t s) {
  hipLaunchKernelGGL(k_obs_gather<RobotList>, dim3(count), dim3(kScanThreads), 0, s, ob, cm, robots);
}
void launch_obs_retransform(const ObsBufDev& ob, const ObsRetransform* items, uint32_t n_items, hipStream_t s) {
  hipLaunchKernelGGL(k_obs_retransform, dim3((ob.max_cloud_points + kScanThreads - 1) / kScanThreads, n_items), dim3(kScanThreads), 0, s, ob, items);
}

}  // namespace navgpu
