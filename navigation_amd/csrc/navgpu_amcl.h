// Internal header of the amcl laser update (amcl_kernels.hip, navgpu_amcl.cpp).
// Device layout of a navgpu_amcl handle (filter-major):
//   poses   : double [n][max_samples][3]   pf_sample_t::pose
//   weights : double [n][max_samples]      pf_sample_t::weight
//   w       : double [n][2]                pf_t::w_slow, w_fast
//   maps    : AmclMapDev [n]               one map_t per filter (several filters may point at one map)
//   skip    : obs_count int32 [n][max_beams], obs_mask uint8 [n][max_beams], info int32 [n][2] {active, error}
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/navgpu.h"

namespace navgpu {

constexpr int kAmclMaxBeams = 1024;  // capacity bound of navgpu_amcl_create's max_beams
constexpr int kAmclMaxMapSide = 16384;
constexpr int kAmclMaxFilters = 65535;  // filters are a grid dimension of k_amcl_laser / k_amcl_normalize

struct AmclMapDev {  // map_t (map.h:57-80)
  const int8_t* occ;  // occ_state per cell: -1 free, 0 unknown, +1 occupied
  const float* dist;  // distances: every map has them (set_map computes them, set_distance_map replaces them)
  int32_t sx, sy;
  double scale, ox, oy, max_occ_dist;
};

struct AmclFilterDev {  // one filter of an update: its sample set and AMCLLaserData after subsampling
  int32_t sample_count, converged;
  int32_t n_beams;   // subsampled beams (range_count stepped by the model's step)
  int32_t active;    // 0: the filter is skipped (updated != 1)
  uint32_t beam_off; // first {range, bearing} pair of this filter in the beam buffer
  int32_t pad;
  double laser[3];   // laser pose in the robot frame
  double range_max;
};

struct AmclDev {
  double* poses;
  double* weights;
  double* w;
  AmclMapDev* maps;
  int32_t* obs_count;
  uint8_t* obs_mask;
  int32_t* skip_info;
  uint32_t max_samples, max_beams;
};

void launch_amcl_convert(const int8_t* msg, uint32_t width, uint32_t height, int factor, int8_t* occ, int sx, int sy, hipStream_t s);
void launch_amcl_cspace(const int8_t* occ, int sx, int sy, int radius, double scale, double max_occ_dist, int32_t* g, float* dist,
                        hipStream_t s);
void launch_amcl_laser(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                       const double* beams, int max_sample_count, int max_n_beams, int count_pass, hipStream_t s);
void launch_amcl_normalize(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                           hipStream_t s);

}  // namespace navgpu
