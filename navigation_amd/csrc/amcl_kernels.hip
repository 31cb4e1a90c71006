// amcl's laser sensor update on the device, for a batch of particle filters (one per robot).
//   AmclNode::convertMap (amcl/src/amcl_node.cpp:1062-1093)                 k_amcl_convert       one thread per cell
//   map_update_cspace (amcl/src/amcl/map/map_cspace.cpp:120-190)            k_amcl_cspace_cols   nearest occupied cell per column
//                                                                            k_amcl_cspace_rows   windowed min of dx^2 + g^2 per row
//   AMCLLaser::BeamModel / LikelihoodFieldModel / ...Prob / ...Gompertz     k_amcl_laser         one thread per particle
//     (amcl/src/amcl/sensors/amcl_laser.cpp:238-690)
//   ApplyModelToSampleSet's map factors + pf_update_sensor (:184-236,       k_amcl_normalize     one workgroup per filter
//     amcl/src/amcl/pf/pf.c:270-316)
// Every expression keeps the reference's operation order in fp64 (the library is built with -ffp-contract=off).  Each particle
// walks its beams in the reference's order in one lane, so `p += pz*pz*pz` and `log_p += log(pz)` round as the serial loop
// does; the filter's subsampled beams sit in LDS, shared by the workgroup's particles.  Sums over particles are fixed-order
// tree reductions: the same bytes run to run, whatever else is scheduled.
#include <hip/hip_runtime.h>

#include "amcl_laser_model.h"

namespace navgpu {

namespace {
constexpr int kLaserThreads = 256, kNormThreads = 256, kColChunk = 64;
}  // namespace

__global__ void k_amcl_convert(const int8_t* __restrict__ msg, uint32_t width, uint32_t height, int factor, int8_t* __restrict__ occ, int sx,
                               int sy) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)sx * sy) return;
  const int y = (int)(i / sx), x = (int)(i % sx);
  const int8_t v = msg[(size_t)(y / factor) * width + x / factor];
  occ[i] = v == 0 ? -1 : (v == 100 ? 1 : 0);
}

// g[y][x] = |y - y'| of the nearest occupied cell (x, y') with |y - y'| <= window, else INT_MAX.  One lane per (column, chunk
// of kColChunk rows): a forward and a backward scan that start `window` rows outside the chunk.
__global__ void k_amcl_cspace_cols(const int8_t* __restrict__ occ, int sx, int sy, int window, int32_t* __restrict__ g) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y0 = blockIdx.y * kColChunk;
  if (x >= sx || y0 >= sy) return;
  const int y1 = min(y0 + kColChunk, sy);
  int last = -1;
  bool seen = false;
  for (int y = max(0, y0 - window); y < y1; ++y) {
    if (occ[x + (size_t)y * sx] == 1) {
      last = y;
      seen = true;
    }
    if (y >= y0) g[x + (size_t)y * sx] = (seen && y - last <= window) ? y - last : INT_MAX;
  }
  seen = false;
  int next = 0;
  for (int y = min(sy - 1, y1 - 1 + window); y >= y0; --y) {
    if (occ[x + (size_t)y * sx] == 1) {
      next = y;
      seen = true;
    }
    if (y < y1 && seen && next - y <= window) {
      int32_t* c = g + x + (size_t)y * sx;
      *c = min(*c, next - y);
    }
  }
}

// D = min over |dx| <= window of dx^2 + g[y][x + dx]^2 (the exact squared distance whenever it is <= radius^2), written
// as map_cspace.cpp's enqueue writes it: (float)(sqrt(D) * scale) within the radius, (float)max_occ_dist beyond
__global__ void k_amcl_cspace_rows(const int32_t* __restrict__ g, int sx, int sy, int window, int radius, double scale, double max_occ_dist,
                                   float* __restrict__ dist) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= sx) return;
  const int32_t* row = g + (size_t)y * sx;
  const int g0 = row[x];
  int best = g0 == INT_MAX ? INT_MAX : g0 * g0;
  for (int k = 1; k <= window && k * k < best; ++k) {
    const int kk = k * k;
    if (x - k >= 0) {
      const int gl = row[x - k];
      if (gl != INT_MAX) best = min(best, kk + gl * gl);
    }
    if (x + k < sx) {
      const int gr = row[x + k];
      if (gr != INT_MAX) best = min(best, kk + gr * gr);
    }
  }
  float out = (float)max_occ_dist;
  if (best != INT_MAX && (int64_t)best <= (int64_t)radius * radius) out = (float)(sqrt((double)best) * scale);
  dist[x + (size_t)y * sx] = out;
}

// One lane per particle j of filter first + blockIdx.y.  count_pass = 1: the beam-skip counting pass of
// LikelihoodFieldModelProb (obs_count per beam, integer atomics); 0: the model itself (weight *= p).
__global__ __launch_bounds__(kLaserThreads) void k_amcl_laser(AmclDev d, navgpu_amcl_laser_params P, uint32_t first,
                                                              const AmclFilterDev* __restrict__ filters, const double* __restrict__ beams,
                                                              int count_pass) {
  extern __shared__ double smem[];
  __shared__ int s_skipped_error;
  const int k = blockIdx.y, tid = threadIdx.x;
  const AmclFilterDev fd = filters[k];
  if (!fd.active) return;
  const uint32_t f = first + k;
  const int nb = fd.n_beams, mb = P.max_beams;
  const bool beamskip = P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB && P.do_beamskip && fd.converged;
  if (count_pass && !beamskip) return;
  double* s_beam = smem;                                   // [nb][2] {range, bearing}
  int* s_int = reinterpret_cast<int*>(smem + 2 * nb);      // [mb] obs_count (count pass) / obs_mask (model pass)
  for (int b = tid; b < 2 * nb; b += blockDim.x) s_beam[b] = beams[2 * (size_t)fd.beam_off + b];
  if (P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB)
    for (int b = tid; b < mb; b += blockDim.x) s_int[b] = 0;
  __syncthreads();

  const AmclMapDev m = d.maps[f];
  const double range_max = fd.range_max;
  const int j = blockIdx.x * blockDim.x + tid;
  const bool live = j < fd.sample_count;
  double pose[3];
  if (live) {
    const double* sp = d.poses + ((size_t)f * d.max_samples + j) * 3;
    const double spose[3] = {sp[0], sp[1], sp[2]};
    coordAdd(fd.laser, spose, pose);
  }

  if (P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB) {
    const double z_hit_denom = 2 * P.sigma_hit * P.sigma_hit;
    const double z_rand_mult = 1.0 / range_max;
    const double max_dist_prob = exp(-(m.max_occ_dist * m.max_occ_dist) / z_hit_denom);
    if (count_pass) {
      if (live)
        for (int b = 0; b < nb; ++b) {
          const double r = s_beam[2 * b];
          if (r >= range_max || r != r) continue;
          bool agrees;
          (void)probPz(P, m, pose, r, s_beam[2 * b + 1], z_hit_denom, z_rand_mult, max_dist_prob, &agrees);
          if (agrees) atomicAdd(&s_int[b], 1);
        }
      __syncthreads();
      for (int b = tid; b < nb; b += blockDim.x)
        if (s_int[b]) atomicAdd(&d.obs_count[(size_t)f * d.max_beams + b], s_int[b]);
      return;
    }
    bool use_error = false;
    if (beamskip) {  // amcl_laser.cpp:543-566, recomputed identically by every workgroup of the filter
      const int32_t* oc = d.obs_count + (size_t)f * d.max_beams;
      for (int b = tid; b < mb; b += blockDim.x) s_int[b] = (oc[b] / static_cast<double>(fd.sample_count)) > P.beam_skip_threshold;
      __syncthreads();
      if (tid == 0) {
        int skipped = 0;
        for (int b = 0; b < mb; ++b) skipped += !s_int[b];
        s_skipped_error = skipped >= (mb * P.beam_skip_error_threshold);
      }
      __syncthreads();
      use_error = s_skipped_error;
    }
    if (blockIdx.x == 0) {
      for (int b = tid; b < mb; b += blockDim.x) d.obs_mask[(size_t)f * d.max_beams + b] = beamskip ? (uint8_t)s_int[b] : 0;
      if (tid == 0) {
        d.skip_info[2 * f] = beamskip;
        d.skip_info[2 * f + 1] = beamskip && use_error;
      }
    }
    if (!live) return;
    const double log_p = probLogP(P, m, s_beam, nb, range_max, pose, z_hit_denom, z_rand_mult, max_dist_prob, beamskip, use_error, s_int);
    d.weights[(size_t)f * d.max_samples + j] *= exp(log_p);
    return;
  }
  if (!live) return;

  const double p = modelP(P, m, s_beam, nb, range_max, pose);
  d.weights[(size_t)f * d.max_samples + j] *= p;
}

namespace {
// Fixed-order sum of v[0..n): lane t adds t, t + 256, ... in order, then a fixed tree over the lanes
__device__ double blockSum(const double* v, int n, double* s_red) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int j = tid; j < n; j += kNormThreads) acc += v[j];
  s_red[tid] = acc;
  __syncthreads();
  for (int w = kNormThreads / 2; w > 0; w >>= 1) {
    if (tid < w) s_red[tid] += s_red[tid + w];
    __syncthreads();
  }
  const double total = s_red[0];
  __syncthreads();
  return total;
}
}  // namespace

// One workgroup per filter: the map factors (ApplyModelToSampleSet :184-233, only when the model's total is > 0), then
// pf_update_sensor's normalisation and running averages (pf.c:280-313)
__global__ __launch_bounds__(kNormThreads) void k_amcl_normalize(AmclDev d, navgpu_amcl_laser_params P, uint32_t first,
                                                                 const AmclFilterDev* __restrict__ filters) {
  __shared__ double s_red[kNormThreads];
  const int k = blockIdx.x, tid = threadIdx.x;
  const AmclFilterDev fd = filters[k];
  if (!fd.active) return;
  const uint32_t f = first + k;
  const int n = fd.sample_count;
  double* wt = d.weights + (size_t)f * d.max_samples;
  double total = blockSum(wt, n, s_red);
  if (total > 0.0) {
    const AmclMapDev m = d.maps[f];
    const double* poses = d.poses + (size_t)f * d.max_samples * 3;
    for (int j = tid; j < n; j += kNormThreads) wt[j] = mapFactor(P, m, poses[3 * j], poses[3 * j + 1], wt[j]);
    __syncthreads();
    total = blockSum(wt, n, s_red);
  }
  if (total > 0.0) {
    double w_avg = total;  // the same weights summed again (pf.c:286-290)
    for (int j = tid; j < n; j += kNormThreads) wt[j] /= total;
    if (tid == 0) {
      w_avg /= n;
      double* w = d.w + 2 * (size_t)f;
      if (w[0] == 0.0)
        w[0] = w_avg;
      else
        w[0] += P.alpha_slow * (w_avg - w[0]);
      if (w[1] == 0.0)
        w[1] = w_avg;
      else
        w[1] += P.alpha_fast * (w_avg - w[1]);
    }
  } else {
    for (int j = tid; j < n; j += kNormThreads) wt[j] = 1.0 / n;
  }
}

void launch_amcl_convert(const int8_t* msg, uint32_t width, uint32_t height, int factor, int8_t* occ, int sx, int sy, hipStream_t s) {
  (void)height;
  const size_t cells = (size_t)sx * sy;
  hipLaunchKernelGGL(k_amcl_convert, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, msg, width, height, factor, occ, sx, sy);
}

void launch_amcl_cspace(const int8_t* occ, int sx, int sy, int radius, double scale, double max_occ_dist, int32_t* g, float* dist, hipStream_t s) {
  const int window = min(radius, max(sx, sy));  // no occupied cell is farther than this along either axis
  hipLaunchKernelGGL(k_amcl_cspace_cols, dim3((sx + 63) / 64, (sy + kColChunk - 1) / kColChunk), dim3(64), 0, s, occ, sx, sy, window, g);
  hipLaunchKernelGGL(k_amcl_cspace_rows, dim3((sx + 255) / 256, sy), dim3(256), 0, s, g, sx, sy, window, radius, scale, max_occ_dist, dist);
}

void launch_amcl_laser(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                       const double* beams, int max_sample_count, int max_n_beams, int count_pass, hipStream_t s) {
  const size_t lds = sizeof(double) * 2 * (size_t)max_n_beams + sizeof(int) * (size_t)max(p.max_beams, 1);
  const unsigned bx = (unsigned)max(1, (max_sample_count + kLaserThreads - 1) / kLaserThreads);
  hipLaunchKernelGGL(k_amcl_laser, dim3(bx, count), dim3(kLaserThreads), lds, s, d, p, first, filters, beams, count_pass);
}

void launch_amcl_normalize(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_amcl_normalize, dim3(count), dim3(kNormThreads), 0, s, d, p, first, filters);
}

}  // namespace navgpu
