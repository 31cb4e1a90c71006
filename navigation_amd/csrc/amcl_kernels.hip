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

#include "navgpu_amcl.h"

namespace navgpu {

namespace {
constexpr int kLaserThreads = 256, kNormThreads = 256, kColChunk = 64;
constexpr double kCellClamp = 536870912.0;  // 2^29: map coordinates are clamped here before the int conversion

// MAP_GXWX / MAP_GYWY + MAP_VALID (map.h:143-149); validity is decided on the double so that no out-of-range conversion happens
__device__ __forceinline__ bool mapCell(const AmclMapDev& m, double x, double y, int& mi, int& mj) {
  const double gx = floor((x - m.ox) / m.scale + 0.5) + (m.sx / 2);
  const double gy = floor((y - m.oy) / m.scale + 0.5) + (m.sy / 2);
  if (!(gx >= 0.0 && gx < (double)m.sx && gy >= 0.0 && gy < (double)m.sy)) return false;
  mi = (int)gx;
  mj = (int)gy;
  return true;
}
__device__ __forceinline__ int mapCoord(const AmclMapDev& m, double v, double origin, int size) {
  const double g = floor((v - origin) / m.scale + 0.5) + (size / 2);
  return (int)fmin(fmax(g, -kCellClamp), kCellClamp);
}
__device__ __forceinline__ bool hitsAt(const AmclMapDev& m, int i, int j) {
  return !(i >= 0 && i < m.sx && j >= 0 && j < m.sy) || m.occ[i + (size_t)j * m.sx] > -1;
}

// map_calc_range (map/map_range.c:37-120): Bresenham from the pose's cell towards the max-range end cell; unknown and
// off-map cells are hits.  The walk leaves the map after at most max(size_x, size_y) + 1 steps, so it always ends.
__device__ double calcRange(const AmclMapDev& m, double ox, double oy, double oa, double max_range) {
  int x0 = mapCoord(m, ox, m.ox, m.sx), y0 = mapCoord(m, oy, m.oy, m.sy);
  int x1 = mapCoord(m, ox + max_range * cos(oa), m.ox, m.sx), y1 = mapCoord(m, oy + max_range * sin(oa), m.oy, m.sy);
  const bool steep = abs(y1 - y0) > abs(x1 - x0);
  if (steep) {
    int t = x0; x0 = y0; y0 = t;
    t = x1; x1 = y1; y1 = t;
  }
  const int deltax = abs(x1 - x0), deltay = abs(y1 - y0);
  int error = 0;
  const int deltaerr = deltay;
  int x = x0, y = y0;
  const int xstep = x0 < x1 ? 1 : -1, ystep = y0 < y1 ? 1 : -1;
  if (steep ? hitsAt(m, y, x) : hitsAt(m, x, y)) return sqrt((double)((x - x0) * (x - x0) + (y - y0) * (y - y0))) * m.scale;
  while (x != (x1 + xstep * 1)) {
    x += xstep;
    error += deltaerr;
    if (2 * error >= deltax) {
      y += ystep;
      error -= deltax;
    }
    if (steep ? hitsAt(m, y, x) : hitsAt(m, x, y)) return sqrt((double)((x - x0) * (x - x0) + (y - y0) * (y - y0))) * m.scale;
  }
  return max_range;
}

// pf_vector_coord_add(laser_pose, sample pose) (pf/pf_vector.c:106-116)
__device__ __forceinline__ void coordAdd(const double* a, const double* b, double* c) {
  const double cb = cos(b[2]), sb = sin(b[2]);
  c[0] = b[0] + a[0] * cb - a[1] * sb;
  c[1] = b[1] + a[0] * sb + a[1] * cb;
  c[2] = b[2] + a[2];
  c[2] = atan2(sin(c[2]), cos(c[2]));
}

// The likelihood-field beam end: map cell of pose + range along pose[2] + bearing; z = its obstacle distance
__device__ __forceinline__ bool beamEnd(const AmclMapDev& m, const double* pose, double r, double bearing, float& z) {
  const double hx = pose[0] + r * cos(pose[2] + bearing);
  const double hy = pose[1] + r * sin(pose[2] + bearing);
  int mi, mj;
  if (!mapCell(m, hx, hy, mi, mj)) return false;
  z = m.dist[mi + (size_t)mj * m.sx];
  return true;
}

// LikelihoodFieldModelProb's pz of one valid beam (amcl_laser.cpp:488-523); *agrees: on the map and closer than
// beam_skip_distance (the obs_count condition)
__device__ __forceinline__ double probPz(const navgpu_amcl_laser_params& P, const AmclMapDev& m, const double* pose, double r, double bearing,
                                        double z_hit_denom, double z_rand_mult, double max_dist_prob, bool* agrees) {
  double pz = 0.0;
  float zf;
  *agrees = false;
  if (!beamEnd(m, pose, r, bearing, zf)) {
    pz += P.z_hit * max_dist_prob;
  } else {
    const double z = zf;
    if (z < P.beam_skip_distance) *agrees = true;
    pz += P.z_hit * exp(-(z * z) / z_hit_denom);
  }
  pz += P.z_rand * z_rand_mult;
  return pz;
}
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
    double log_p = 0;
    for (int b = 0; b < nb; ++b) {
      const double r = s_beam[2 * b];
      if (r >= range_max || r != r) continue;
      if (beamskip && !(use_error || s_int[b])) continue;  // only entries written in this update are integrated
      bool agrees;
      log_p += log(probPz(P, m, pose, r, s_beam[2 * b + 1], z_hit_denom, z_rand_mult, max_dist_prob, &agrees));
    }
    d.weights[(size_t)f * d.max_samples + j] *= exp(log_p);
    return;
  }
  if (!live) return;

  double p;
  if (P.model_type == NAVGPU_AMCL_MODEL_BEAM) {  // amcl_laser.cpp:238-303
    p = 1.0;
    for (int b = 0; b < nb; ++b) {
      const double obs_range = s_beam[2 * b], obs_bearing = s_beam[2 * b + 1];
      const double map_range = calcRange(m, pose[0], pose[1], pose[2] + obs_bearing, range_max);
      double pz = 0.0;
      const double z = obs_range - map_range;
      pz += P.z_hit * exp(-(z * z) / (2 * P.sigma_hit * P.sigma_hit));
      if (z < 0) pz += P.z_short * P.lambda_short * exp(-P.lambda_short * obs_range);
      if (obs_range == range_max) pz += P.z_max * 1.0;
      if (obs_range < range_max) pz += P.z_rand * 1.0 / range_max;
      p += pz * pz * pz;
    }
  } else if (P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD) {  // :305-380
    p = 1.0;
    const double z_hit_denom = 2 * P.sigma_hit * P.sigma_hit;
    const double z_rand_mult = 1.0 / range_max;
    for (int b = 0; b < nb; ++b) {
      const double obs_range = s_beam[2 * b];
      if (obs_range >= range_max) continue;
      if (obs_range != obs_range) continue;
      double pz = 0.0;
      float zf;
      const double z = beamEnd(m, pose, obs_range, s_beam[2 * b + 1], zf) ? (double)zf : m.max_occ_dist;
      pz += P.z_hit * exp(-(z * z) / z_hit_denom);
      pz += P.z_rand * z_rand_mult;
      p += pz * pz * pz;
    }
  } else {  // LikelihoodFieldModelGompertz :605-690 and applyGompertz :593-603
    const double z_hit_denom = 2 * P.sigma_hit * P.sigma_hit;
    int valid_beams = 0;
    double sum_pz = 0.0;
    for (int b = 0; b < nb; ++b) {
      const double obs_range = s_beam[2 * b];
      if (obs_range >= range_max) continue;
      if (obs_range != obs_range) continue;
      valid_beams++;
      double pz = 0.0;
      float zf;
      const double z = beamEnd(m, pose, obs_range, s_beam[2 * b + 1], zf) ? (double)zf : m.max_occ_dist;
      pz += P.z_hit * exp(-(z * z) / z_hit_denom);
      pz += P.z_rand;
      sum_pz += pz;
    }
    if (valid_beams > 0) {
      p = sum_pz / valid_beams;
      p = p * P.input_scale + P.input_shift;
      p = P.gompertz_a * exp(-1.0 * P.gompertz_b * exp(-1.0 * P.gompertz_c * p));
      p += P.output_shift;
    } else {
      p = 1.0;
    }
  }
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
    for (int j = tid; j < n; j += kNormThreads) {
      int mi, mj;
      double w = wt[j];
      if (!mapCell(m, poses[3 * j], poses[3 * j + 1], mi, mj)) {
        w *= P.off_map_factor;
      } else if (m.occ[mi + (size_t)mj * m.sx] != -1) {
        w *= P.non_free_space_factor;
      } else if (m.dist[mi + (size_t)mj * m.sx] < P.non_free_space_radius) {
        const double delta_d = m.dist[mi + (size_t)mj * m.sx] / P.non_free_space_radius;
        double fac = P.non_free_space_factor;
        fac += delta_d * (1.0 - P.non_free_space_factor);
        w *= fac;
      }
      wt[j] = w;
    }
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
