// GlobalPlanner::makePlan around its core (navfn_kernels.hip: k_gp_plan, k_gp_wf_finish), for a batch of plans:
//   k_gp_clear_cells     clearRobotCell                                   (planner_core.cpp:176-185, 283-286)
//   k_gp_plan_scan       where each plan begins in the concatenated output
//   k_gp_plan_emit       getPlanFromPotential + goal_copy + OrientationFilter::processPath on yaws
//                                                                        (planner_core.cpp:306-312, 351-395, orientation_filter.cpp:53-111)
//   k_gp_potential_grid  publishPotential's data                          (planner_core.cpp:417-434)
// All pose arithmetic is fp64 with the reference's operation order (-ffp-contract=off: no fused multiply-add).
#include "global_plan_kernels.h"
#include "navfn_rules.h"

namespace navgpu {

constexpr int kGpThreads = 256, kGpWaves = kGpThreads / 64;

__global__ void k_gp_clear_cells(NavfnDev nv, uint32_t first, uint32_t count, const int32_t* cells) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int32_t cell = cells[k];
  if (cell < 0 || cell >= nv.ns) return;
  nv.costarr[(size_t)(first + k) * nv.ns_padded + cell] = 0;  // costmap_2d::FREE_SPACE
}

// One workgroup: plans in chunks of 256, each chunk scanned by waves (__shfl_up) with one LDS word per wave, the running total
// carried from chunk to chunk.  No atomics: the offsets are a pure function of the records.
__global__ __launch_bounds__(kGpThreads) void k_gp_plan_scan(const GpPlanRec* recs, uint32_t count, uint32_t* offsets) {
  __shared__ uint32_t wave_total[kGpWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < count; base += kGpThreads) {
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < count ? (uint32_t)max(recs[k].n_poses, 0) : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = carry, chunk = 0;
#pragma unroll
    for (int w = 0; w < kGpWaves; ++w) {
      if (w < wave) before += wave_total[w];
      chunk += wave_total[w];
    }
    if (k < count) offsets[k] = before + incl - v;
    carry += chunk;
    __syncthreads();  // wave_total is rewritten by the next chunk
  }
  if (threadIdx.x == 0) offsets[count] = carry;
}

// angles::shortest_angular_distance, the fmod form of normalize_angle (navgpu_shortest_angular_distance on the host)
__device__ __forceinline__ double gpShortestAngularDistance(double from, double to) {
  double r = fmod(fmod(to - from, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI);
  if (r > M_PI) r -= 2.0 * M_PI;
  return r;
}

// pose i of a plan before the orientation filter: the traceback's point n_path - 1 - i through mapToWorld (planner_core.cpp:196-199),
// the float promoted first; behind the traceback's points, the goal
struct GpPlanView {
  const float *px, *py;
  GpPlanRec r;
  __device__ __forceinline__ double x(int i) const {
    return i < r.n_path ? r.origin_x + ((double)px[r.n_path - 1 - i] + r.convert_offset) * r.resolution : r.goal_x;
  }
  __device__ __forceinline__ double y(int i) const {
    return i < r.n_path ? r.origin_y + ((double)py[r.n_path - 1 - i] + r.convert_offset) * r.resolution : r.goal_y;
  }
  __device__ __forceinline__ double yaw0(int i) const { return i < r.n_path ? 0.0 : r.goal_yaw; }
  // OrientationFilter::pointToNext (orientation_filter.cpp:89-98), i <= n_poses - 2: from the two positions' own expressions, so
  // that every lane that needs this angle gets the same bits
  __device__ __forceinline__ double forward(int i) const { return atan2(y(i + 1) - y(i), x(i + 1) - x(i)); }
};

// One workgroup per plan; lane t takes poses t, t + 256, ... so consecutive lanes write consecutive poses.
__global__ __launch_bounds__(kGpThreads) void k_gp_plan_emit(NavfnDev nv, uint32_t first, const GpPlanRec* recs, const uint32_t* offsets,
                                                             navgpu_global_pose* poses, uint32_t capacity) {
  __shared__ int wave_best[kGpWaves];
  GpPlanView p;
  p.r = recs[blockIdx.x];
  const int n = p.r.n_poses - (p.r.has_tail ? 1 : 0), mode = p.r.mode;  // the planner's own plan; a tail pose goes behind it untouched
  if (n <= 0) return;  // (the whole workgroup)
  p.px = nv.path + (size_t)(first + blockIdx.x) * 2 * nv.path_cap;
  p.py = p.px + nv.path_cap;
  const uint32_t base = offsets[blockIdx.x];
  // (the whole workgroup) nothing of this plan fits.  In 64 bits, as below: kPpNoWrite, the offset of a plan that a handover keeps out
  // of its robot's slot (navgpu_device.h), is 0xFFFFFFFF and capacity at most that.
  if ((uint64_t)base >= capacity) return;
  if (p.r.has_tail && threadIdx.x == 0 && (uint64_t)base + n < capacity) poses[base + n] = navgpu_global_pose{p.r.tail_x, p.r.tail_y, p.r.tail_yaw};
  const bool forward = mode == NAVGPU_ORIENT_FORWARD || mode == NAVGPU_ORIENT_FORWARD_THEN_INTERPOLATE;
  const bool search = mode == NAVGPU_ORIENT_FORWARD_THEN_INTERPOLATE && n >= 3;
  const double last = search ? p.forward(n - 3) : 0.0;
  // INTERPOLATE: interpolate(0, n - 1) from the start's yaw is known before any pose is
  const double whole_inc = gpShortestAngularDistance(p.r.start_yaw, p.r.goal_yaw) / (n - 1);
  int best = 0;  // the search's result as a maximum: the largest j in [1, n - 3] with |sad(yaw[j - 1], last)| > 0.35, or 0
  for (int i = threadIdx.x; i < n; i += kGpThreads) {
    double yaw = p.yaw0(i);
    if (forward && i < n - 1) yaw = p.forward(i);
    if (mode == NAVGPU_ORIENT_INTERPOLATE) yaw = p.r.start_yaw + whole_inc * i;
    if (search && i + 1 <= n - 3 && fabs(gpShortestAngularDistance(yaw, last)) > 0.35) best = max(best, i + 1);
    if ((uint64_t)base + i < capacity) poses[base + i] = navgpu_global_pose{p.x(i), p.y(i), yaw};
  }
  if (mode != NAVGPU_ORIENT_FORWARD_THEN_INTERPOLATE) return;  // (the whole workgroup)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d, 64));
  if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
  __syncthreads();
  int a = 0;
#pragma unroll
  for (int w = 0; w < kGpWaves; ++w) a = max(a, wave_best[w]);
  // path[0] takes the start's orientation, then interpolate(a, n - 1) (orientation_filter.cpp:83-84, 100-111): each lane
  // rewrites the poses it wrote itself
  const double start_yaw = a == 0 ? p.r.start_yaw : p.forward(a);
  const double inc = gpShortestAngularDistance(start_yaw, p.r.goal_yaw) / (n - 1 - a);
  for (int i = threadIdx.x; i < n; i += kGpThreads) {
    if ((uint64_t)base + i >= capacity) break;
    if (i >= a)
      poses[base + i].yaw = start_yaw + inc * i;
    else if (i == 0)
      poses[base].yaw = p.r.start_yaw;
  }
}

// One workgroup per plan: the maximum of the potentials below POT_HIGH (a maximum of floats: exact whatever the order), then the
// bytes.  Lanes stride over the row-major array, so loads and stores are coalesced and any cell count is covered.
__global__ __launch_bounds__(kGpThreads) void k_gp_potential_grid(NavfnDev nv, uint32_t first, const uint8_t* use_alt, int32_t publish_scale,
                                                                  int8_t* grids, float* maxima) {
  __shared__ float wave_max[kGpWaves];
  const uint32_t plan = first + blockIdx.x;
  const float* potential = (use_alt[blockIdx.x] ? nv.potalt : nv.potarr) + (size_t)plan * nv.ns_padded;
  int8_t* grid = grids + (size_t)blockIdx.x * nv.ns;
  float mx = 0.0f;
  for (int i = threadIdx.x; i < nv.ns; i += kGpThreads) {
    const float v = potential[i];
    if (v < kPotHigh && v > mx) mx = v;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = 0.0f;
#pragma unroll
  for (int w = 0; w < kGpWaves; ++w) mx = fmaxf(mx, wave_max[w]);
  if (threadIdx.x == 0) maxima[blockIdx.x] = mx;
  for (int i = threadIdx.x; i < nv.ns; i += kGpThreads) {
    const float v = potential[i];
    int8_t out = -1;
    if (!(v >= kPotHigh)) out = mx == 0.0f ? (int8_t)0 : (int8_t)truncX86(v * publish_scale / mx);  // float * int -> float, float / float
    grid[i] = out;
  }
}

void launch_gp_clear_cells(const NavfnDev& nv, uint32_t first, uint32_t count, const int32_t* cells, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_clear_cells, dim3((count + 255) / 256), dim3(256), 0, s, nv, first, count, cells);
}
void launch_gp_plan_scan(const GpPlanRec* recs, uint32_t count, uint32_t* offsets, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_plan_scan, dim3(1), dim3(kGpThreads), 0, s, recs, count, offsets);
}
void launch_gp_plan_emit(const NavfnDev& nv, uint32_t first, uint32_t count, const GpPlanRec* recs, const uint32_t* offsets, navgpu_global_pose* poses,
                         uint32_t capacity, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_plan_emit, dim3(count), dim3(kGpThreads), 0, s, nv, first, recs, offsets, poses, capacity);
}
void launch_gp_potential_grid(const NavfnDev& nv, uint32_t first, uint32_t count, const uint8_t* use_alt, int32_t publish_scale, int8_t* grids,
                              float* maxima, hipStream_t s) {
  hipLaunchKernelGGL(k_gp_potential_grid, dim3(count), dim3(kGpThreads), 0, s, nv, first, use_alt, publish_scale, grids, maxima);
}

}  // namespace navgpu
