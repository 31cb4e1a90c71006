// navfn::NavfnROS round its NavFn (navfn_kernels.hip), for a batch of plans:
//   k_nr_window           makePlan's tolerance search / validPointPotential's        (navfn_ros.cpp:301-327, 130-155)
//   k_nr_path             getPlanFromPotential's calcPath(nx * 4)                    (:426-437)
//   k_nr_point_potential  getPointPotential                                          (:157-169)
//   k_nr_cloud_count / k_nr_cloud_scan / k_nr_cloud_emit   the `potential` cloud    (:342-368)
// Costs and coordinates are fp64 with the reference's operation order (-ffp-contract=off: no fused multiply-add).  Nothing here
// places or chooses anything with an atomic: every output is a pure function of the inputs.
#include "navfn_ros_kernels.h"

#include <cfloat>

#include "global_plan_kernels.h"
#include "navfn_calc_path.h"

namespace navgpu {

constexpr int kNrThreads = 256, kNrWaves = kNrThreads / 64;

__device__ __forceinline__ const float* nrPotential(const NavfnDev& nv, uint32_t plan, int use_alt) {
  return (use_alt ? nv.potalt : nv.potarr) + (size_t)plan * nv.ns_padded;
}

// One workgroup per window.  Lane t takes the candidates t, t + 256, ... of the scan order iy * nx + ix, keeps the first of its
// lowest cost, and the workgroup reduces to the minimum of (cost, scan index): the candidate the reference's strict
// `cost < best_cost` from DBL_MAX keeps in y-outer / x-inner order.  A cost that is not below DBL_MAX (inf, NaN) never wins.
template <bool kAnyOnly>
__global__ __launch_bounds__(kNrThreads) void k_nr_window(NavfnDev nv, uint32_t first, const NrWindow* windows, const double* seq, NrBest* best) {
  __shared__ double wave_cost[kNrWaves];
  __shared__ int wave_index[kNrWaves];
  __shared__ int wave_count[kNrWaves];
  const NrWindow w = windows[blockIdx.x];
  const float* potarr = nrPotential(nv, first + w.plan, w.use_alt);
  const double* ys = seq + w.seq;
  const double* xs = ys + w.ny;
  const uint32_t n = w.ny * w.nx;  // <= 4096 * 4096
  double cost = DBL_MAX;
  int index = -1, count = 0;
  for (uint32_t i = threadIdx.x; i < n; i += kNrThreads) {
    const uint32_t iy = i / w.nx, ix = i - iy * w.nx;
    const double px = xs[ix], py = ys[iy];
    int32_t cell[2];
    if (!costmapWorldToMap(px, py, w.origin_x, w.origin_y, w.resolution, nv.nx, nv.ny, cell)) continue;  // getPointPotential: DBL_MAX
    const float potential = potarr[cell[1] * nv.nx + cell[0]];
    if (!(potential < kPotHigh)) continue;
    ++count;
    if (kAnyOnly) continue;
    const double dx = px - w.goal_x, dy = py - w.goal_y;  // sq_distance (navfn_ros.h:181-185)
    const double c = sqrt(dx * dx + dy * dy) * w.w_dist + (double)potential * w.w_len;
    if (c < cost) {  // (ascending i within a lane: the first of equal costs stays)
      cost = c;
      index = (int)i;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double oc = __shfl_xor(cost, d, 64);
    const int oi = __shfl_xor(index, d, 64);
    count += __shfl_xor(count, d, 64);
    if (oi >= 0 && (index < 0 || oc < cost || (oc == cost && oi < index))) {
      cost = oc;
      index = oi;
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    wave_cost[wave] = cost;
    wave_index[wave] = index;
    wave_count[wave] = count;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  cost = DBL_MAX, index = -1, count = 0;
#pragma unroll
  for (int v = 0; v < kNrWaves; ++v) {
    count += wave_count[v];
    const double oc = wave_cost[v];
    const int oi = wave_index[v];
    if (oi >= 0 && (index < 0 || oc < cost || (oc == cost && oi < index))) {
      cost = oc;
      index = oi;
    }
  }
  NrBest b{};
  b.index = index;
  b.candidates = kAnyOnly ? (count > 0) : count;
  b.cost = cost;
  if (index >= 0) {
    const uint32_t iy = (uint32_t)index / w.nx, ix = (uint32_t)index - iy * w.nx;
    b.x = xs[ix];
    b.y = ys[iy];
    costmapWorldToMap(b.x, b.y, w.origin_x, w.origin_y, w.resolution, nv.nx, nv.ny, b.cell);
  }
  best[blockIdx.x] = b;
}

// One wave per plan, lane 0 walks (calcPath is a sequential process; the batch is the parallel dimension, as in k_navfn_plan).
__global__ __launch_bounds__(64) void k_nr_path(NavfnDev nv, uint32_t first, NrPathJob* jobs, const NrBest* best) {
  if (threadIdx.x != 0) return;
  const uint32_t plan = first + blockIdx.x;
  NrPathJob j = jobs[blockIdx.x];
  j.first_pass = nv.results[plan];
  j.length = 0;
  if (j.from_best) {
    const NrBest b = best[blockIdx.x];
    j.start[0] = b.index >= 0 ? b.cell[0] : -1;
    j.start[1] = b.index >= 0 ? b.cell[1] : -1;
  }
  if (j.start[0] >= 0) {
    const float* potarr = nrPotential(nv, plan, j.use_alt);
    const int start_cell = j.start[1] * nv.nx + j.start[0];
    // A walk that STARTS on cell (0, 1) or (0, ny - 1) reads one element outside potarr in the reference unless it ends at once.  A
    // border cell is unreached unless it is the robot's, its (int) potential is INT_MIN, no neighbour is lower and the walk ends
    // with "high potential" whatever those elements hold short of a NaN: restated as that end, without the reads.  Only the start
    // is covered: a walk that ARRIVES on one of these two cells reads those elements, as it does in k_navfn_plan (navfnCalcPath's
    // own bounds test is the reference's, `stc < nx || stc > ns - nx`); border cells are unreached on every array NavFn leaves.
    const bool outside = (start_cell == nv.nx || start_cell == nv.ns - nv.nx) && potarr[start_cell] >= kPotHigh;
    if (!outside) {
      navfnCalcPath(nv, plan, potarr, j.goal[0], j.goal[1], j.start[0], j.start[1], nv.nx * 4, j.first_pass.cycles);
      j.length = nv.results[plan].path_length;
    } else {
      navgpu_navfn_result r = j.first_pass;
      r.found = 0;
      r.path_length = 0;
      r.start_potential = potarr[start_cell];
      nv.results[plan] = r;
    }
  }
  jobs[blockIdx.x] = j;
}

__global__ __launch_bounds__(kNrThreads) void k_nr_point_potential(NavfnDev nv, uint32_t first, const NrCloudPlan* plans, const int32_t* qplan,
                                                                   double* xy, uint32_t n_queries) {
  const uint32_t q = blockIdx.x * kNrThreads + threadIdx.x;
  if (q >= n_queries) return;
  const int32_t k = qplan[q];
  const NrCloudPlan p = plans[k];
  int32_t cell[2];
  double out = DBL_MAX;
  if (costmapWorldToMap(xy[2 * q], xy[2 * q + 1], p.origin_x, p.origin_y, p.resolution, nv.nx, nv.ny, cell))
    out = (double)nrPotential(nv, first + k, p.use_alt)[cell[1] * nv.nx + cell[0]];
  xy[2 * q] = out;
}

// ------------------------------------------------------------------------------------------------ the potential cloud
// An order-preserving compaction laid out as voxel_export_kernels.hip's: (a) a workgroup per (chunk of 1024 cells, plan) counts,
// (b) one workgroup scans all the totals in (plan, chunk) order, (c) as (a), each lane recomputing its offset in the chunk.
// A lane takes 4 consecutive cells with one 16-byte load (a plan's array begins at a multiple of 64 floats), so a wave reads
// 1 KiB contiguously, and lane order = cell order = the reference's loop order.

// Exclusive prefix of v over the workgroup's lanes in lane order, and the workgroup's total
__device__ __forceinline__ uint32_t nrBlockExclusive(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)kNrWaves; ++w) {
    const uint32_t t = s_wave[w];
    before += w < wave ? t : 0u;
    total += t;
  }
  __syncthreads();  // s_wave may be written again
  return before + inc - v;
}

// the lane's 4 potentials and which of them the cloud keeps (`pp[i] < 10e7`, the float promoted, :357)
__device__ __forceinline__ uint32_t nrLaneCells(const NavfnDev& nv, const float* potarr, uint32_t c0, float v[4]) {
  uint32_t keep = 0;
  if (c0 >= (uint32_t)nv.ns) return 0;  // c0 is a multiple of 4 below ns <= ns_padded, a multiple of 64: the 16 bytes are the plan's own
  const float4 q = *reinterpret_cast<const float4*>(potarr + c0);
  v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    if (c0 + j < (uint32_t)nv.ns && (double)v[j] < 10e7) keep |= 1u << j;
  return keep;
}

__global__ __launch_bounds__(kNrThreads) void k_nr_cloud_count(NavfnDev nv, uint32_t first, const NrCloudPlan* plans, uint32_t* totals) {
  __shared__ uint32_t s_wave[kNrWaves];
  const uint32_t k = blockIdx.y;
  float v[4];
  const uint32_t keep = nrLaneCells(nv, nrPotential(nv, first + k, plans[k].use_alt), blockIdx.x * kNrChunk + threadIdx.x * 4, v);
  uint32_t total;
  nrBlockExclusive(__popc(keep), s_wave, total);
  if (threadIdx.x == 0) totals[(size_t)k * gridDim.x + blockIdx.x] = total;
}

// one workgroup: the totals become their exclusive prefix in tiles of 256 with a carry; offsets[k] = the prefix plan k begins with
__global__ __launch_bounds__(kNrThreads) void k_nr_cloud_scan(uint32_t* totals, uint32_t chunks, uint32_t count, uint32_t* offsets) {
  __shared__ uint32_t s_wave[kNrWaves];
  const uint32_t n = chunks * count;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += kNrThreads) {  // (uniform: every lane runs every tile)
    const uint32_t i = base + threadIdx.x;
    const uint32_t mine = i < n ? totals[i] : 0u;
    uint32_t tile;
    const uint32_t ex = nrBlockExclusive(mine, s_wave, tile);
    if (i < n) {
      totals[i] = carry + ex;
      if (i % chunks == 0) offsets[i / chunks] = carry + ex;
    }
    carry += tile;
  }
  if (threadIdx.x == 0) offsets[count] = carry;
}

__global__ __launch_bounds__(kNrThreads) void k_nr_cloud_emit(NavfnDev nv, uint32_t first, const NrCloudPlan* plans, const uint32_t* totals,
                                                              NrCloudPoint* points, uint32_t capacity) {
  __shared__ uint32_t s_wave[kNrWaves];
  const uint32_t k = blockIdx.y;
  const NrCloudPlan p = plans[k];
  const float* potarr = nrPotential(nv, first + k, p.use_alt);
  const uint32_t c0 = blockIdx.x * kNrChunk + threadIdx.x * 4;
  float v[4];
  const uint32_t keep = nrLaneCells(nv, potarr, c0, v);
  uint32_t total;
  uint32_t at = totals[(size_t)k * gridDim.x + blockIdx.x] + nrBlockExclusive(__popc(keep), s_wave, total);
  if (!keep) return;
  const float divisor = potarr[p.start_cell];  // pp[start[1] * nx + start[0]]
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    if (!(keep >> j & 1u)) continue;
    if (at >= capacity) return;
    const uint32_t c = c0 + j, my = c / (uint32_t)nv.nx, mx = c - my * (uint32_t)nv.nx;
    NrCloudPoint pt;
    pt.x = (float)(p.origin_x + (double)mx * p.resolution);  // mapToWorld (:208-211), narrowed by the assignment
    pt.y = (float)(p.origin_y + (double)my * p.resolution);
    pt.z = v[j] / divisor * 20;
    pt.pot_value = v[j];
    points[at++] = pt;
  }
}

void launch_nr_window(const NavfnDev& nv, uint32_t first, const NrWindow* windows, const double* seq, uint32_t n_windows, int any_only, NrBest* best,
                      hipStream_t s) {
  if (any_only)
    hipLaunchKernelGGL(k_nr_window<true>, dim3(n_windows), dim3(kNrThreads), 0, s, nv, first, windows, seq, best);
  else
    hipLaunchKernelGGL(k_nr_window<false>, dim3(n_windows), dim3(kNrThreads), 0, s, nv, first, windows, seq, best);
}
void launch_nr_path(const NavfnDev& nv, uint32_t first, uint32_t count, NrPathJob* jobs, const NrBest* best, hipStream_t s) {
  hipLaunchKernelGGL(k_nr_path, dim3(count), dim3(64), 0, s, nv, first, jobs, best);
}
void launch_nr_point_potential(const NavfnDev& nv, uint32_t first, const NrCloudPlan* plans, const int32_t* qplan, double* xy, uint32_t n_queries,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_nr_point_potential, dim3((n_queries + kNrThreads - 1) / kNrThreads), dim3(kNrThreads), 0, s, nv, first, plans, qplan, xy,
                     n_queries);
}
void launch_nr_cloud_count(const NavfnDev& nv, uint32_t first, uint32_t count, const NrCloudPlan* plans, uint32_t* totals, uint32_t* offsets,
                           hipStream_t s) {
  const uint32_t chunks = nrCloudChunks(nv.ns);
  hipLaunchKernelGGL(k_nr_cloud_count, dim3(chunks, count), dim3(kNrThreads), 0, s, nv, first, plans, totals);
  hipLaunchKernelGGL(k_nr_cloud_scan, dim3(1), dim3(kNrThreads), 0, s, totals, chunks, count, offsets);
}
void launch_nr_cloud_emit(const NavfnDev& nv, uint32_t first, uint32_t count, const NrCloudPlan* plans, const uint32_t* totals, NrCloudPoint* points,
                          uint32_t capacity, hipStream_t s) {
  hipLaunchKernelGGL(k_nr_cloud_emit, dim3(nrCloudChunks(nv.ns), count), dim3(kNrThreads), 0, s, nv, first, plans, totals, points, capacity);
}

}  // namespace navgpu
