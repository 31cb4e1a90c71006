// amcl's odometry motion model on the device, for a batch of particle filters.
//   AMCLOdom::UpdateAction (amcl/src/amcl/sensors/amcl_odom.cpp:128-379): all five models, one lane per particle
//   pf_ran_gaussian (pf/pf_pdf.c:132-146) over drand48(): k_amcl_drand48_gauss, one workgroup per filter
// pf_ran_gaussian's rejection loop consumes a data-dependent but fully determined number of drand48() values: values equal to 0.0
// are skipped, the others pair up consecutively as (x1, x2), and a pair is accepted when 0 < w = x1*x1 + x2*x2 <= 1 (exact IEEE
// arithmetic).  That is a stream compaction: lanes generate the stream in rounds by LCG jump-ahead, the nonzero values are scanned
// into a compacted list, the pairs are tested, and the accepted pairs are scanned into record indices.  A record is
// (x2, sqrt(-2.0*log(w)/w)) rather than a unit deviate because the reference multiplies sigma * x2 first.  Everything that depends
// on the odometry alone comes from the host (AmclOdomFilterDev::k); only per-particle sin / cos / atan2 (and log in the records)
// are the device's.  fp64 throughout, no contraction (the Makefile's -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "navgpu_amcl.h"

namespace navgpu {

namespace {
constexpr int kGaussThreads = 256;
constexpr int kGaussWaves = kGaussThreads / 64;
constexpr int kPerLane = 8;                                      // drand48 values per lane per round
constexpr int kRound = kGaussThreads * kPerLane;                 // values per round
constexpr int kPairsPerLane = (kRound + 1 + 2 * kGaussThreads - 1) / (2 * kGaussThreads);  // pairs of a round (with the carry)
constexpr int kOdomThreads = 256;
constexpr uint64_t kMask48 = (1ull << 48) - 1;
constexpr uint64_t kLcgA = 0x5DEECE66Dull, kLcgC = 0xB;

// X -> A X + C (mod 2^48) as the pair (A, C); 64-bit products wrap mod 2^64, a multiple of 2^48
struct Affine {
  uint64_t a, c;
};
__device__ __forceinline__ Affine compose(Affine f, Affine g) {  // g after f
  return Affine{(g.a * f.a) & kMask48, (g.a * f.c + g.c) & kMask48};
}
// the generator advanced k steps
__device__ Affine jump(uint32_t k) {
  Affine r{1, 0}, b{kLcgA, kLcgC};
  while (k) {
    if (k & 1) r = compose(r, b);
    b = compose(b, b);
    k >>= 1;
  }
  return r;
}

// exclusive prefix sum of one int per thread over the workgroup; every thread calls it
__device__ int blockScan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  int pre = 0, tot = 0;
  for (int w = 0; w < kGaussWaves; ++w) {
    const int s = wsum[w];
    if (w < wv) pre += s;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return pre + x - v;
}

// 3 * sample_count records of one filter in the reference's draw order; the state comes back advanced past the last value used
__global__ __launch_bounds__(kGaussThreads) void k_amcl_drand48_gauss(double2* records, uint32_t max_samples, AmclOdomFilterDev* filters) {
  AmclOdomFilterDev* F = filters + blockIdx.x;
  if (!F->active || F->sample_count <= 0) return;
  __shared__ uint64_t sv[kRound + 2];  // the round's nonzero values as LCG states, after the carried one
  __shared__ int wsum[kGaussWaves];
  __shared__ uint64_t s_x, s_next, s_carry_state, s_final;
  __shared__ int s_carry, s_rec;
  const int t = threadIdx.x;
  const int need = 3 * F->sample_count;
  double2* rec = records + (size_t)blockIdx.x * 3 * max_samples;
  const Affine lane_jump = jump((uint32_t)(t * kPerLane));
  if (t == 0) {
    s_x = F->state;
    s_carry = 0;
    s_rec = 0;
  }
  __syncthreads();
  for (;;) {
    // 1. this lane's kPerLane values of the round
    uint64_t x = (lane_jump.a * s_x + lane_jump.c) & kMask48;
    uint64_t st[kPerLane];
    int nz = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      x = (kLcgA * x + kLcgC) & kMask48;
      st[k] = x;
      nz += x != 0;
    }
    // 2. compact the nonzero values (r == 0.0 exactly when the state is 0) behind the carried one
    int total = 0;
    int pos = s_carry + blockScan(nz, wsum, total);
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
      if (st[k] != 0) sv[pos++] = st[k];
    if (t == kGaussThreads - 1) s_next = x;
    if (t == 0 && s_carry) sv[0] = s_carry_state;
    __syncthreads();
    // 3. pairs (sv[2p], sv[2p + 1]), kPairsPerLane consecutive pairs per lane; accepted ones become records in order
    const int nsurv = s_carry + total, npairs = nsurv >> 1;
    double x2v[kPairsPerLane], wv[kPairsPerLane];
    int acc = 0;
    unsigned ok = 0;
#pragma unroll
    for (int j = 0; j < kPairsPerLane; ++j) {
      const int p = t * kPairsPerLane + j;
      wv[j] = 2.0;
      x2v[j] = 0.0;
      if (p < npairs) {
        const double x1 = 2.0 * ((double)sv[2 * p] * 0x1p-48) - 1.0;
        const double x2 = 2.0 * ((double)sv[2 * p + 1] * 0x1p-48) - 1.0;
        const double w = x1 * x1 + x2 * x2;
        x2v[j] = x2;
        wv[j] = w;
        if (!(w > 1.0 || w == 0.0)) {
          ok |= 1u << j;
          ++acc;
        }
      }
    }
    int accepted = 0;
    int idx = s_rec + blockScan(acc, wsum, accepted);
#pragma unroll
    for (int j = 0; j < kPairsPerLane; ++j) {
      if (!(ok >> j & 1)) continue;
      if (idx < need) {
        const double w = wv[j];
        rec[idx] = make_double2(x2v[j], sqrt(-2.0 * log(w) / w));
        if (idx == need - 1) s_final = sv[2 * (t * kPairsPerLane + j) + 1];
      }
      ++idx;
    }
    __syncthreads();
    if (t == 0) {
      s_rec += accepted;
      s_carry = nsurv & 1;
      if (s_carry) s_carry_state = sv[nsurv - 1];
      s_x = s_next;
    }
    __syncthreads();
    if (s_rec >= need) break;
  }
  if (t == 0) F->state = s_final;
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
