// Internal header of the amcl laser update (amcl_kernels.hip, navgpu_amcl.cpp).
// Device layout of a navgpu_amcl handle (filter-major):
//   poses   : double [n][max_samples][3]   pf_sample_t::pose
//   weights : double [n][max_samples]      pf_sample_t::weight
//   w       : double [n][2]                pf_t::w_slow, w_fast
//   maps    : AmclMapDev [n]               one map_t per filter (several filters may point at one map)
//   skip    : obs_count int32 [n][max_beams], obs_mask uint8 [n][max_beams], info int32 [n][2] {active, error}
// Resampling (amcl_resample_kernels.hip) adds a per-filter workspace (AmclResampleDev) and the cluster statistics of the
// current set: cl_count int32 [n][max_samples], cl_stats double [n][max_samples][13] {weight, mean[3], cov[9]},
// set_stats double [n][12] {mean[3], cov[9]}.
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
  const int32_t* free_cells;  // cell indices i + j * sx of occ_state == -1, x-major (amcl_node.cpp:1028-1033); for random poses
  int32_t n_free;
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

// Resampling of one filter of an update_resample call (pf_update_resample and what it calls, pf.c:319-588)
struct AmclResampleFilterDev {
  // in
  int32_t sample_count;  // set a
  int32_t leaf_in;       // kd-tree leaf count of set a at its creation (systematic)
  int32_t pool_count;    // supplied random poses of this filter
  int32_t active;
  uint64_t pool_off;     // first pose of this filter in the pool (supplied draws)
  uint64_t rng_ctr;      // per-filter call counter (device draws)
  double sys_start;      // systematic_sample_start (supplied draws)
  // out
  int32_t status;        // NAVGPU_OK or NAVGPU_ERR_INVALID (nothing written then)
  int32_t count;         // set b's sample_count
  int32_t leaf_out;      // set b's leaf count
  int32_t converged;     // pf_update_converged
  int32_t cluster_count;
  int32_t n_random;      // samples drawn from the random-pose source
};

struct AmclResampleParamsDev {
  int32_t model, min_samples, max_samples, draw_device;
  double pop_err, pop_z, dist_threshold;
  uint64_t seed;
};

// Workspace of every filter, sized for max_samples (P = next power of two >= max_samples sort slots)
struct AmclResampleDev {
  uint32_t P;
  double* c;           // [n][max_samples + 1] cumulative table; reused for the systematic targets
  double* cand;        // [n][max_samples][3] candidate poses (set b before the stop)
  double* cs;          // [n][max_samples][2] cos, sin of set b's angles
  uint64_t* skey;      // [n][P] sort keys
  uint32_t* sidx;      // [n][P] sort payload (sample index)
  int32_t* a;          // [n][max_samples] flags / scans
  int32_t* b;          // [n][max_samples] bin of each sample / cluster of each sample
  int32_t* label;      // [n][max_samples] component label of each bin (its lowest sample index)
  uint64_t* ukey;      // [n][max_samples] occupied bins of set b, ascending
  int32_t* cstart;     // [n][max_samples] first position of each cluster in the second sort
  const double* u;     // supplied {u_flag, u_pick} pairs: [count][max_samples][2] (multinomial)
  const double* pool;  // supplied random poses
  int32_t* cl_count;
  double* cl_stats;
  double* set_stats;
};

void launch_amcl_resample(const AmclDev& d, const AmclResampleDev& r, const AmclResampleParamsDev& p, uint32_t first, uint32_t count,
                          AmclResampleFilterDev* filters, hipStream_t s);

void launch_amcl_convert(const int8_t* msg, uint32_t width, uint32_t height, int factor, int8_t* occ, int sx, int sy, hipStream_t s);
void launch_amcl_cspace(const int8_t* occ, int sx, int sy, int radius, double scale, double max_occ_dist, int32_t* g, float* dist,
                        hipStream_t s);
void launch_amcl_laser(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                       const double* beams, int max_sample_count, int max_n_beams, int count_pass, hipStream_t s);
void launch_amcl_normalize(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                           hipStream_t s);

}  // namespace navgpu
