// amcl's odometry motion model on the device, for a batch of particle filters.
//   AMCLOdom::UpdateAction (amcl/src/amcl/sensors/amcl_odom.cpp:128-379): all five models, one lane per particle
//   pf_ran_gaussian (pf/pf_pdf.c:132-146) over drand48(): k_amcl_drand48_gauss, one workgroup per filter
// The records are amcl_drand48.h's: (x2, sqrt(-2.0*log(w)/w)) per deviate, in the reference's draw order.  Everything that depends
// on the odometry alone comes from the host (AmclOdomFilterDev::k); only per-particle sin / cos / atan2 (and log in the records)
// are the device's.  fp64 throughout, no contraction (the Makefile's -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "amcl_drand48.h"

namespace navgpu {

namespace {
constexpr int kOdomThreads = 256;

// 3 * sample_count records of one filter in the reference's draw order; the state comes back advanced past the last value used
__global__ __launch_bounds__(kGaussThreads) void k_amcl_drand48_gauss(double2* records, uint32_t max_samples, AmclOdomFilterDev* filters) {
  AmclOdomFilterDev* F = filters + blockIdx.x;
  if (!F->active || F->sample_count <= 0) return;
  drand48GaussRecords(records + (size_t)blockIdx.x * 3 * max_samples, 3 * F->sample_count, &F->state);
}

__device__ __forceinline__ double normalizeAngle(double z) { return atan2(sin(z), cos(z)); }
// amcl_odom.cpp's angle_diff(a, b) with a already normalised (on the host)
__device__ __forceinline__ double angleDiffN(double a, double b) {
  b = normalizeAngle(b);
  const double d1 = a - b;
  double d2 = 2 * M_PI - fabs(d1);
  if (d1 > 0) d2 *= -1.0;
  if (fabs(d1) < fabs(d2)) return d1;
  return d2;
}

__global__ __launch_bounds__(kOdomThreads) void k_amcl_odom(AmclDev d, int32_t model, int32_t dev, uint64_t seed, const double2* records,
                                                            uint32_t first, const AmclOdomFilterDev* filters) {
  const AmclOdomFilterDev& F = filters[blockIdx.y];
  const int i = blockIdx.x * kOdomThreads + threadIdx.x;
  if (!F.active || i >= F.sample_count) return;
  const uint32_t f = first + blockIdx.y;
  const size_t ms = d.max_samples;
  // the particle's three deviates in the model's draw order: (x2, s) records, or Box-Muller on two Philox draws
  double g[3][2];
  if (dev) {
    double u0, u1, u2, u3;
    draw2(seed, f, F.rng_ctr, 2 * (uint32_t)i, 2, u0, u1);
    draw2(seed, f, F.rng_ctr, 2 * (uint32_t)i + 1, 2, u2, u3);
    const double r0 = sqrt(-2.0 * log(1.0 - u0)), r1 = sqrt(-2.0 * log(1.0 - u2));
    g[0][0] = r0 * cos(2 * M_PI * u1);
    g[1][0] = r0 * sin(2 * M_PI * u1);
    g[2][0] = r1 * cos(2 * M_PI * u3);
  } else {
    const double2* r = records + (size_t)blockIdx.y * 3 * ms + 3 * (size_t)i;
    for (int j = 0; j < 3; ++j) {
      const double2 v = r[j];
      g[j][0] = v.x;
      g[j][1] = v.y;
    }
  }
  // pf_ran_gaussian(sigma): sigma * x2 * s, left to right; device draws: sigma * z
  auto gauss = [&](int j, double sigma) { return dev ? sigma * g[j][0] : sigma * g[j][0] * g[j][1]; };
  double* pose = d.poses + ((size_t)f * ms + i) * 3;
  double p0 = pose[0], p1 = pose[1], p2 = pose[2];
  const double* k = F.k;
  if (model == NAVGPU_AMCL_ODOM_DIFF || model == NAVGPU_AMCL_ODOM_DIFF_CORRECTED) {
    // k = {normalize(delta_rot1), normalize(delta_rot2), delta_trans, sd_rot1, sd_trans, sd_rot2}
    const double rot1_hat = angleDiffN(k[0], gauss(0, k[3]));
    const double trans_hat = k[2] - gauss(1, k[4]);
    const double rot2_hat = angleDiffN(k[1], gauss(2, k[5]));
    p0 += trans_hat * cos(p2 + rot1_hat);
    p1 += trans_hat * sin(p2 + rot1_hat);
    p2 += rot1_hat + rot2_hat;
  } else if (model == NAVGPU_AMCL_ODOM_OMNI || model == NAVGPU_AMCL_ODOM_OMNI_CORRECTED) {
    // k = {bearing, delta_trans, delta_rot, sd_trans, sd_rot, sd_strafe}
    const double bearing = k[0] + p2;
    const double cs = cos(bearing), sn = sin(bearing);
    const double trans_hat = k[1] + gauss(0, k[3]);
    const double rot_hat = k[2] + gauss(1, k[4]);
    const double strafe_hat = 0 + gauss(2, k[5]);
    p0 += (trans_hat * cs + strafe_hat * sn);
    p1 += (trans_hat * sn - strafe_hat * cs);
    p2 += rot_hat;
  } else {
    // k = {bearing, delta_trans, delta_rot, delta.v[2] / 2, sd_trans, sd_strafe, sd_rot}
    const double heading = p2 + k[3];
    const double cs_h = cos(heading), sn_h = sin(heading);
    const double bearing = k[0] + p2;
    const double cs_b = cos(bearing), sn_b = sin(bearing);
    const double trans_hat = gauss(0, k[4]);
    const double strafe_hat = gauss(1, k[5]);
    const double rot_hat = gauss(2, k[6]);
    p0 += (k[1] * cs_b);
    p1 += (k[1] * sn_b);
    p2 += k[2];
    p0 += (trans_hat * cs_h + strafe_hat * sn_h);
    p1 += (trans_hat * sn_h - strafe_hat * cs_h);
    p2 += rot_hat;
  }
  pose[0] = p0;
  pose[1] = p1;
  pose[2] = p2;
}
}  // namespace

void launch_amcl_drand48_gauss(double2* records, uint32_t max_samples, uint32_t count, AmclOdomFilterDev* filters, hipStream_t s) {
  hipLaunchKernelGGL(k_amcl_drand48_gauss, dim3(count), dim3(kGaussThreads), 0, s, records, max_samples, filters);
}

void launch_amcl_odom(const AmclDev& d, int32_t model, int32_t draw_device, uint64_t seed, const double2* records, uint32_t first,
                      uint32_t count, int max_sample_count, const AmclOdomFilterDev* filters, hipStream_t s) {
  if (max_sample_count <= 0) return;
  const unsigned blocks = (unsigned)((max_sample_count + kOdomThreads - 1) / kOdomThreads);
  hipLaunchKernelGGL(k_amcl_odom, dim3(blocks, count), dim3(kOdomThreads), 0, s, d, model, draw_device, seed, records, first, filters);
}

}  // namespace navgpu
