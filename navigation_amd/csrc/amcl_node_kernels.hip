// AmclNode::laserReceived's two device pieces that are not pf steps (navgpu_amcl_node_laser_received, navgpu_amcl_hypotheses):
//   the scan conversion (amcl/src/amcl_node.cpp:1524-1537)     k_amcl_scan         one workgroup per filter
//   the hypothesis read-out (amcl/src/amcl_node.cpp:1584-1651)  k_amcl_hypothesis   one wave per filter
// Both are a few hundred bytes of work per filter and bound by launch latency; they exist so that a cycle neither builds beams on
// the host (16 B per ray over the bus, 4 B here) nor waits for the stream between its steps.
// fp64 with the reference's operation order: the library is built with -ffp-contract=off, so `angle_min + (i * angle_increment)`
// rounds the product before the sum, as the reference's x86-64 build does.
#include <hip/hip_runtime.h>

#include "navgpu_amcl.h"

namespace navgpu {

namespace {
constexpr int kScanThreads = 64, kHypThreads = 64;  // one wave each
}

// Filter k of the slice: beams[beam_off + j] = {range, bearing} of ray i = j * step, j < n_beams (the models' subsampled rays:
// every model walks `for (i = 0; i < range_count; i += step)`), and the beam-skip state of the filter cleared as update_sensor
// clears it before the model runs.
__global__ __launch_bounds__(kScanThreads) void k_amcl_scan(AmclDev d, uint32_t first, const AmclFilterDev* __restrict__ filters,
                                                            const AmclScanDev* __restrict__ scans, const float* __restrict__ raw,
                                                            double* __restrict__ beams) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const AmclScanDev sc = scans[k];
  if (!sc.active) return;
  const AmclFilterDev fd = filters[k];
  const uint32_t f = first + k;
  for (uint32_t b = tid; b < d.max_beams; b += kScanThreads) {
    d.obs_count[(size_t)f * d.max_beams + b] = 0;
    d.obs_mask[(size_t)f * d.max_beams + b] = 0;
  }
  if (tid < 2) d.skip_info[2 * (size_t)f + tid] = 0;
  const float* ranges = raw + sc.range_off;
  double* out = beams + 2 * (size_t)fd.beam_off;
  for (int j = tid; j < fd.n_beams; j += kScanThreads) {
    const int64_t i64 = (int64_t)j * sc.step;
    if (i64 >= sc.range_count) break;  // n_beams = ceil(range_count / step): never taken
    const int i = (int)i64;
    const float r = ranges[i];
    // "amcl doesn't (yet) have a concept of min range.  So we'll map short readings to max range."  A NaN fails the test.
    double range;
    if ((double)r <= sc.range_min)
      range = sc.range_max;
    else
      range = (double)r;
    out[2 * j] = range;
    out[2 * j + 1] = sc.angle_min + ((double)i * sc.angle_inc);
  }
}

// Filter k of the slice: the first cluster with the strictly largest weight above 0, in the device's cluster order (clusters are
// numbered by their lowest sample index), its mean, and the set's covariance entries.  Lane l looks at clusters l, l + 64, ...
// in order and keeps the first strict maximum; the butterfly then keeps the larger weight and, of equal weights, the lower
// index: the same winner as the serial loop `if (weight > max_weight)` over 0 .. cluster_count - 1.  No atomics.
__global__ __launch_bounds__(kHypThreads) void k_amcl_hypothesis(AmclResampleDev r, uint32_t max_samples, uint32_t first,
                                                                 const AmclResampleFilterDev* __restrict__ rfilters,
                                                                 AmclHypDev* __restrict__ hyps) {
  const int k = blockIdx.x, lane = threadIdx.x;
  AmclHypDev* H = hyps + k;
  if (!H->active) return;
  const uint32_t f = first + k;
  int C = H->cluster_count;
  if (H->from_resample && rfilters[k].status == NAVGPU_OK) C = rfilters[k].cluster_count;
  if (C < 0) C = 0;
  if ((uint32_t)C > max_samples) C = (int)max_samples;
  const double* st = r.cl_stats + (size_t)f * max_samples * 13;
  double best = 0.0;
  int idx = -1;
  for (int c = lane; c < C; c += kHypThreads) {
    const double w = st[13 * (size_t)c];
    if (w > best) {
      best = w;
      idx = c;
    }
  }
  for (int off = kHypThreads / 2; off > 0; off >>= 1) {
    const double ow = __shfl_xor(best, off, kHypThreads);
    const int oi = __shfl_xor(idx, off, kHypThreads);
    if (ow > best || (ow == best && oi >= 0 && (idx < 0 || oi < idx))) {
      best = ow;
      idx = oi;
    }
  }
  if (lane == 0) {
    H->clusters = C;
    H->max_weight_hyp = idx;
    H->max_weight = best;
  }
  if (lane < 3) H->pose[lane] = idx >= 0 ? st[13 * (size_t)idx + 1 + lane] : 0.0;
  if (lane < 5) {
    // pf_sample_set_t::cov.m[0][0], [0][1], [1][0], [1][1], [2][2] of {mean[3], cov[9]}
    const int at[5] = {3, 4, 6, 7, 11};
    H->cov[lane] = r.set_stats[12 * (size_t)f + at[lane]];
  }
}

void launch_amcl_scan(const AmclDev& d, uint32_t first, uint32_t count, const AmclFilterDev* filters, const AmclScanDev* scans,
                      const float* raw, double* beams, hipStream_t s) {
  hipLaunchKernelGGL(k_amcl_scan, dim3(count), dim3(kScanThreads), 0, s, d, first, filters, scans, raw, beams);
}

void launch_amcl_hypothesis(const AmclResampleDev& r, uint32_t max_samples, uint32_t first, uint32_t count,
                            const AmclResampleFilterDev* rfilters, AmclHypDev* hyps, hipStream_t s) {
  hipLaunchKernelGGL(k_amcl_hypothesis, dim3(count), dim3(kHypThreads), 0, s, r, max_samples, first, rfilters, hyps);
}

}  // namespace navgpu
