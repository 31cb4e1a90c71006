// Per-pose pieces of amcl's laser model, shared by k_amcl_laser / k_amcl_normalize (amcl_kernels.hip) and the scored uniform
// init (amcl_init_kernels.hip).  The expressions are the reference's, in its operation order (fp64, no contraction).
#pragma once
#include <hip/hip_runtime.h>

#include "navgpu_amcl.h"

namespace navgpu {
namespace {
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

// BeamModel / LikelihoodFieldModel / LikelihoodFieldModelGompertz's p of one sample (amcl_laser.cpp:238-380, 593-690); pose is
// pf_vector_coord_add(laser pose, sample pose), beams the subsampled {range, bearing} pairs
__device__ __forceinline__ double modelP(const navgpu_amcl_laser_params& P, const AmclMapDev& m, const double* s_beam, int nb,
                                         double range_max, const double* pose) {
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
  return p;
}

// LikelihoodFieldModelProb's log p of one sample (amcl_laser.cpp:525-590); with beamskip, only the beams of mask (or all, on
// use_error) are integrated
__device__ __forceinline__ double probLogP(const navgpu_amcl_laser_params& P, const AmclMapDev& m, const double* s_beam, int nb,
                                           double range_max, const double* pose, double z_hit_denom, double z_rand_mult,
                                           double max_dist_prob, bool beamskip, bool use_error, const int* mask) {
  double log_p = 0;
  for (int b = 0; b < nb; ++b) {
    const double r = s_beam[2 * b];
    if (r >= range_max || r != r) continue;
    if (beamskip && !(use_error || mask[b])) continue;  // only entries written in this update are integrated
    bool agrees;
    log_p += log(probPz(P, m, pose, r, s_beam[2 * b + 1], z_hit_denom, z_rand_mult, max_dist_prob, &agrees));
  }
  return log_p;
}

// ApplyModelToSampleSet's map factors of one sample at (x, y) (amcl_laser.cpp:197-233)
__device__ __forceinline__ double mapFactor(const navgpu_amcl_laser_params& P, const AmclMapDev& m, double x, double y, double w) {
  int mi, mj;
  if (!mapCell(m, x, y, mi, mj)) {
    w *= P.off_map_factor;
  } else if (m.occ[mi + (size_t)mj * m.sx] != -1) {
    w *= P.non_free_space_factor;
  } else if (m.dist[mi + (size_t)mj * m.sx] < P.non_free_space_radius) {
    const double delta_d = m.dist[mi + (size_t)mj * m.sx] / P.non_free_space_radius;
    double fac = P.non_free_space_factor;
    fac += delta_d * (1.0 - P.non_free_space_factor);
    w *= fac;
  }
  return w;
}
}  // namespace
}  // namespace navgpu
