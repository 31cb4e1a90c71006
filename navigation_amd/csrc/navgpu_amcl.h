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
// The motion model (amcl_motion_kernels.hip) adds, in drand48 mode, a record workspace: double2 [n][3 max_samples] {x2, s}.
// The init (amcl_init_kernels.hip) uses the resampling workspace and, for the Gaussian in drand48 mode, the record workspace.
// The node cycle (amcl_node_kernels.hip) adds per-filter scan and hypothesis records (AmclScanDev, AmclHypDev [n]) and the raw
// float ranges of the last call; its beams go into the sensor update's beam buffer.
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

// Philox4x32-10 (Salmon et al., SC'11): counter {draw index, filter | stream << 16, call counter lo, hi}, key = seed.  Streams:
// 0 and 1 resampling (amcl_resample_kernels.hip), 2 the motion model (amcl_motion_kernels.hip), 3 the Gaussian init and 4 the
// uniform init (amcl_init_kernels.hip; stream 4 puts the retry number where the counter's high word would be).
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// two doubles in [0, 1) with 53 random bits each
__device__ __forceinline__ void draw2(uint64_t seed, uint32_t filter, uint64_t call, uint32_t index, uint32_t stream,
                                      double& u0, double& u1) {
  uint32_t c[4] = {index, filter | (stream << 16), (uint32_t)call, (uint32_t)(call >> 32)};
  philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double s = 1.0 / 9007199254740992.0;
  u0 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * s;
  u1 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6)) * s;
}

void launch_amcl_resample(const AmclDev& d, const AmclResampleDev& r, const AmclResampleParamsDev& p, uint32_t first, uint32_t count,
                          AmclResampleFilterDev* filters, hipStream_t s);

// One filter of an update_action call (AMCLOdom::UpdateAction, amcl_odom.cpp:128-379).  k[] holds what depends on the odometry
// alone, computed on the host in the reference's own expressions (navgpu_amcl.cpp, odomConstants):
//   diff / diff-corrected: {normalize(delta_rot1), normalize(delta_rot2), delta_trans, sd_rot1, sd_trans, sd_rot2}
//   omni / omni-corrected: {bearing, delta_trans, delta_rot, sd_trans, sd_rot, sd_strafe}
//   Gaussian:              {bearing, delta_trans, delta_rot, delta.v[2] / 2, sd_trans, sd_strafe, sd_rot}
// with bearing = angle_diff(atan2(delta.v[1], delta.v[0]), old_pose.v[2]).
struct AmclOdomFilterDev {
  int32_t sample_count;
  int32_t active;        // 0: the filter is skipped (invalid drand48 state)
  uint64_t state;        // drand48 mode: the 48-bit LCG state, in and out
  uint64_t rng_ctr;      // device mode: the filter's call counter
  double k[7];
};

constexpr int kAmclOdomConsts = 7;
constexpr uint64_t kAmclDrand48Mask = (1ull << 48) - 1;  // drand48's state is 48 bits

void launch_amcl_drand48_gauss(double2* records, uint32_t max_samples, uint32_t count, AmclOdomFilterDev* filters, hipStream_t s);
void launch_amcl_odom(const AmclDev& d, int32_t model, int32_t draw_device, uint64_t seed, const double2* records, uint32_t first,
                      uint32_t count, int max_sample_count, const AmclOdomFilterDev* filters, hipStream_t s);

// One filter of an init call (pf_init / pf_init_model)
struct AmclInitFilterDev {
  int32_t active;        // 0: the filter is skipped
  int32_t status;        // in: NAVGPU_OK; out: NAVGPU_ERR_INVALID (bad bin), NAVGPU_ERR_CAPACITY (candidate cap); nothing written then
  uint64_t state;        // drand48 mode: the 48-bit LCG state (the Gaussian records advance it)
  uint64_t rng_ctr;      // device mode: the filter's call counter
  uint64_t used;         // uniform, scored: candidates drawn (out)
  const int32_t* free_cells;  // uniform: the free cells of this call
  int32_t n_free;
  int32_t n_beams;       // scored: subsampled beams of the scan
  uint32_t beam_off;     // scored: first {range, bearing} pair in the beam buffer
  int32_t leaf_out, cluster_count;  // out
  int32_t pad;
  double mean[3], cr[9], cd[3];     // Gaussian: pf_pdf_gaussian_alloc's x, cr (row-major) and cd
  double laser[3];       // scored: laser pose in the robot frame
  double range_max;
};

struct AmclInitParamsDev {
  int32_t gaussian, draw_device, scored, pad;
  double threshold, multiplier;   // scored: uniform_pose_starting_weight_threshold, uniform_pose_deweight_multiplier
  uint64_t max_candidates;        // per filter (scored)
  uint64_t seed;
};

void launch_amcl_init(const AmclDev& d, const AmclResampleDev& r, const AmclInitParamsDev& p, const navgpu_amcl_laser_params& P,
                      const double* beams, int max_n_beams, double2* records, uint32_t first, uint32_t count, AmclInitFilterDev* filters,
                      hipStream_t s);

// AmclNode's laser cycle (amcl_node_kernels.hip).  One filter's LaserScan as amcl_node.cpp:1505-1537 reads it; filter k of the
// slice writes its subsampled beams where its AmclFilterDev says (beam_off, n_beams)
struct AmclScanDev {
  int32_t active;        // 0: the filter is skipped
  int32_t step;          // the model's subsampling step (>= 1 for an active filter)
  uint32_t range_off;    // first raw range of this filter
  int32_t range_count;
  double range_min, range_max;  // the float thresholds of :1514-1522, widened
  double angle_min, angle_inc;  // :1505-1509
};
// One filter's hypothesis read-out (amcl_node.cpp:1584-1651)
struct AmclHypDev {
  // in
  int32_t active;
  int32_t cluster_count;   // the set's cluster count as the host knows it
  int32_t from_resample;   // 1: this call's resample record of the filter holds the count when its status is NAVGPU_OK
  // out
  int32_t clusters;        // the count that was read
  int32_t max_weight_hyp;  // -1: no cluster with weight > 0
  int32_t pad;
  double max_weight;
  double pose[3];          // hyps[max_weight_hyp].pf_pose_mean
  double cov[5];           // set->cov.m[0][0], [0][1], [1][0], [1][1], [2][2]
};
void launch_amcl_scan(const AmclDev& d, uint32_t first, uint32_t count, const AmclFilterDev* filters, const AmclScanDev* scans,
                      const float* raw, double* beams, hipStream_t s);
void launch_amcl_hypothesis(const AmclResampleDev& r, uint32_t max_samples, uint32_t first, uint32_t count,
                            const AmclResampleFilterDev* rfilters, AmclHypDev* hyps, hipStream_t s);

void launch_amcl_convert(const int8_t* msg, uint32_t width, uint32_t height, int factor, int8_t* occ, int sx, int sy, hipStream_t s);
void launch_amcl_cspace(const int8_t* occ, int sx, int sy, int radius, double scale, double max_occ_dist, int32_t* g, float* dist,
                        hipStream_t s);
void launch_amcl_laser(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                       const double* beams, int max_sample_count, int max_n_beams, int count_pass, hipStream_t s);
void launch_amcl_normalize(const AmclDev& d, const navgpu_amcl_laser_params& p, uint32_t first, uint32_t count, const AmclFilterDev* filters,
                           hipStream_t s);

}  // namespace navgpu
