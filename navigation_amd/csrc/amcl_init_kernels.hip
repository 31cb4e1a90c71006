// amcl's filter initialisation on the device, for a batch of particle filters.
//   pf_init (pf/pf.c:138-176) with pf_pdf_gaussian_sample (pf/pf_pdf.c:105-126)   k_amcl_init_records + k_amcl_init_gauss
//   pf_init_model (pf.c:180-213) with AmclNode::uniformPoseGenerator (amcl_node.cpp:1200-1263)
//     drand48, unscored; device draws                                             k_amcl_init_free     one lane per sample
//     drand48, scored                                                              k_amcl_init_chain    one workgroup per filter
//   the kd-tree histogram and pf_cluster_stats of the new set                      k_amcl_init_set      one workgroup per filter
// The new poses go to the resampling workspace (AmclResampleDev::cand) first; k_amcl_init_set checks every pose's histogram bin
// and only then replaces the filter's set, so a filter that fails is left as it was.
// Draws.  drand48 mode regenerates the reference's stream from the caller's state: the Gaussian records are amcl_drand48.h's
// (3 per sample, sample order); uniform candidate j takes values 2j (cell) and 2j + 1 (theta).  Device mode uses Philox
// (navgpu_amcl.h): stream 3 for the Gaussian, {2i, 2i + 1} per sample i; stream 4 for uniform poses, counter
// {sample, filter | 4 << 16, call counter (low 32 bits), retry}.
// Scoring (scorePose, amcl_node.cpp:1216-1236): the configured laser model on a one-sample set of weight 1.0 with converged = 0
// (no beam skipping), then ApplyModelToSampleSet's map factors when the total is > 0.  The acceptance chain of the scored
// drand48 mode is serial by definition (the threshold restarts at every accepted sample): each round scores 256 candidates, one
// per lane, and one lane walks the round's scores against gw, gw *= multiplier after every rejection, as the reference does.
#include <hip/hip_runtime.h>

#include "amcl_drand48.h"
#include "amcl_laser_model.h"
#include "amcl_pf_stages.h"

namespace navgpu {

namespace {
constexpr int kInitThreads = 256;
constexpr int kChainRound = kInitThreads;  // candidates per round of k_amcl_init_chain

// Philox draws of device-mode uniform poses: {u_cell, u_theta} of retry k of sample i
__device__ __forceinline__ void drawFree(uint64_t seed, uint32_t filter, uint64_t call, uint32_t i, uint32_t k, double& u0, double& u1) {
  uint32_t c[4] = {i, filter | (4u << 16), (uint32_t)call, k};
  philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double s = 1.0 / 9007199254740992.0;
  u0 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * s;
  u1 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6)) * s;
}

// the filter's map with the free-cell list of this call (cells farther than non_free_space_radius from an obstacle)
__device__ __forceinline__ AmclMapDev initMap(const AmclDev& d, uint32_t f, const AmclInitFilterDev& F) {
  AmclMapDev m = d.maps[f];
  m.free_cells = F.free_cells;
  m.n_free = F.n_free;
  return m;
}

// AmclNode::scorePose: the model's weight of a one-sample set (weight 1.0, converged 0), then the map factors when it is > 0
__device__ double scorePose(const navgpu_amcl_laser_params& P, const AmclMapDev& m, const double* s_beam, int nb, double range_max,
                            const double* laser, const double* pose) {
  if (P.max_beams < 2) return 0.0;  // ApplyModelToSampleSet returns 0 (amcl_laser.cpp:184-185)
  double lp[3];
  coordAdd(laser, pose, lp);
  double w = 1.0;
  if (P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB) {
    const double z_hit_denom = 2 * P.sigma_hit * P.sigma_hit;
    const double z_rand_mult = 1.0 / range_max;
    const double max_dist_prob = exp(-(m.max_occ_dist * m.max_occ_dist) / z_hit_denom);
    w *= exp(probLogP(P, m, s_beam, nb, range_max, lp, z_hit_denom, z_rand_mult, max_dist_prob, false, false, nullptr));
  } else {
    w *= modelP(P, m, s_beam, nb, range_max, lp);
  }
  if (w > 0.0) w = mapFactor(P, m, pose[0], pose[1], w);
  return w;
}

__device__ __forceinline__ void loadBeams(double* s_beam, const double* beams, const AmclInitFilterDev& F) {
  for (int b = threadIdx.x; b < 2 * F.n_beams; b += blockDim.x) s_beam[b] = beams[2 * (size_t)F.beam_off + b];
  __syncthreads();
}

// the 3 * max_samples Gaussian records of every filter (drand48 mode); F->state comes back advanced
__global__ __launch_bounds__(kGaussThreads) void k_amcl_init_records(double2* records, uint32_t max_samples, AmclInitFilterDev* filters) {
  AmclInitFilterDev* F = filters + blockIdx.x;
  if (!F->active) return;
  drand48GaussRecords(records + (size_t)blockIdx.x * 3 * max_samples, 3 * (int)max_samples, &F->state);
}

// pf_pdf_gaussian_sample: r[j] = pf_ran_gaussian(cd[j]) for j = 0, 1, 2, then x[i] = mean[i] + sum_j cr[i][j] * r[j] in j order
__global__ __launch_bounds__(kInitThreads) void k_amcl_init_gauss(AmclDev d, AmclResampleDev r, AmclInitParamsDev p, const double2* records,
                                                                  uint32_t first, const AmclInitFilterDev* filters) {
  const AmclInitFilterDev& F = filters[blockIdx.y];
  const int i = blockIdx.x * kInitThreads + threadIdx.x;
  if (!F.active || i >= (int)d.max_samples) return;
  const uint32_t f = first + blockIdx.y;
  double rv[3];
  if (p.draw_device) {  // Box-Muller on two Philox draws, as update_action's device mode
    double u0, u1, u2, u3;
    draw2(p.seed, f, F.rng_ctr, 2 * (uint32_t)i, 3, u0, u1);
    draw2(p.seed, f, F.rng_ctr, 2 * (uint32_t)i + 1, 3, u2, u3);
    const double r0 = sqrt(-2.0 * log(1.0 - u0)), r1 = sqrt(-2.0 * log(1.0 - u2));
    rv[0] = F.cd[0] * (r0 * cos(2 * M_PI * u1));
    rv[1] = F.cd[1] * (r0 * sin(2 * M_PI * u1));
    rv[2] = F.cd[2] * (r1 * cos(2 * M_PI * u3));
  } else {  // sigma * x2 * s, left to right
    const double2* rec = records + (size_t)blockIdx.y * 3 * d.max_samples + 3 * (size_t)i;
    for (int j = 0; j < 3; ++j) {
      const double2 v = rec[j];
      rv[j] = F.cd[j] * v.x * v.y;
    }
  }
  double* out = r.cand + ((size_t)f * d.max_samples + i) * 3;
  for (int a = 0; a < 3; ++a) {
    double x = F.mean[a];
    for (int j = 0; j < 3; ++j) x += F.cr[3 * a + j] * rv[j];
    out[a] = x;
  }
}

// One lane per sample: drand48 unscored (candidate i is sample i) or device draws, each sample retrying on its own while its
// score is below gw (scored).  F->used gets the candidates drawn.
__global__ __launch_bounds__(kInitThreads) void k_amcl_init_free(AmclDev d, AmclResampleDev r, AmclInitParamsDev p, navgpu_amcl_laser_params P,
                                                                 const double* beams, uint32_t first, AmclInitFilterDev* filters) {
  extern __shared__ double s_beam[];
  AmclInitFilterDev* F = filters + blockIdx.y;
  if (!F->active) return;
  if (p.scored) loadBeams(s_beam, beams, *F);
  const int i = blockIdx.x * kInitThreads + threadIdx.x;
  if (i >= (int)d.max_samples) return;
  const uint32_t f = first + blockIdx.y;
  const AmclMapDev m = initMap(d, f, *F);
  double pose[3] = {0.0, 0.0, 0.0};
  if (!p.draw_device) {
    // values 2i and 2i + 1 of the stream: the states 2i + 1 and 2i + 2 steps after F->state
    const Affine j = jump(2 * (uint32_t)i + 1);
    const uint64_t x1 = (j.a * F->state + j.c) & kMask48, x2 = (kLcgA * x1 + kLcgC) & kMask48;
    freePose(m, (double)x1 * 0x1p-48, (double)x2 * 0x1p-48, pose);
  } else {
    // scored: every candidate is counted in F->used at once, and every lane stops as soon as the filter's total passes
    // max_candidates (k_amcl_init_set then reports NAVGPU_ERR_CAPACITY), so a call never draws much beyond the cap
    unsigned long long* used = (unsigned long long*)&F->used;
    uint32_t k = 0;
    double gw = p.threshold;
    for (;;) {
      double uc, ut;
      drawFree(p.seed, f, F->rng_ctr, (uint32_t)i, k, uc, ut);
      freePose(m, uc, ut, pose);
      ++k;
      if (!p.scored) break;
      if (atomicAdd(used, 1ull) >= p.max_candidates) break;  // this candidate is beyond the cap: F->used > max_candidates
      if (!(scorePose(P, m, s_beam, F->n_beams, F->range_max, F->laser, pose) < gw)) break;
      gw *= p.multiplier;
    }
  }
  double* out = r.cand + ((size_t)f * d.max_samples + i) * 3;
  out[0] = pose[0];
  out[1] = pose[1];
  out[2] = pose[2];
}

// drand48, scored: rounds of kChainRound candidates (one per lane: pose and score), then one lane walks the round
__global__ __launch_bounds__(kInitThreads) void k_amcl_init_chain(AmclDev d, AmclResampleDev r, AmclInitParamsDev p, navgpu_amcl_laser_params P,
                                                                  const double* beams, uint32_t first, AmclInitFilterDev* filters) {
  extern __shared__ double s_beam[];
  __shared__ double s_score[kChainRound], s_pose[kChainRound][3];
  __shared__ int s_take[kChainRound];
  __shared__ int s_sample;
  __shared__ double s_gw;
  __shared__ uint64_t s_x, s_used;
  AmclInitFilterDev* F = filters + blockIdx.x;
  if (!F->active) return;
  loadBeams(s_beam, beams, *F);
  const int t = threadIdx.x, ms = (int)d.max_samples;
  const uint32_t f = first + blockIdx.x;
  const AmclMapDev m = initMap(d, f, *F);
  double* cand = r.cand + (size_t)f * ms * 3;
  const Affine lane = jump(2 * (uint32_t)t + 1), round = jump(2 * kChainRound);
  if (t == 0) {
    s_x = F->state;
    s_sample = 0;
    s_gw = p.threshold;
    s_used = 0;
  }
  __syncthreads();
  for (uint64_t base = 0; s_sample < ms && base < p.max_candidates; base += kChainRound) {
    const bool live = base + t < p.max_candidates;
    if (live) {
      const uint64_t x1 = (lane.a * s_x + lane.c) & kMask48, x2 = (kLcgA * x1 + kLcgC) & kMask48;
      freePose(m, (double)x1 * 0x1p-48, (double)x2 * 0x1p-48, s_pose[t]);
      s_score[t] = scorePose(P, m, s_beam, F->n_beams, F->range_max, F->laser, s_pose[t]);
    }
    s_take[t] = -1;
    __syncthreads();
    if (t == 0) {  // uniformPoseGenerator's loop: while (score < gw) { next candidate; gw *= multiplier; }
      int sample = s_sample;
      double gw = s_gw;
      for (int k = 0; k < kChainRound && sample < ms && base + k < p.max_candidates; ++k) {
        if (!(s_score[k] < gw)) {
          s_take[k] = sample++;
          gw = p.threshold;
          s_used = base + k + 1;
        } else {
          gw *= p.multiplier;
        }
      }
      s_sample = sample;
      s_gw = gw;
      s_x = (round.a * s_x + round.c) & kMask48;
    }
    __syncthreads();
    const int q = s_take[t];
    if (q >= 0) {
      cand[3 * (size_t)q] = s_pose[t][0];
      cand[3 * (size_t)q + 1] = s_pose[t][1];
      cand[3 * (size_t)q + 2] = s_pose[t][2];
    }
    __syncthreads();
  }
  if (t == 0) {
    F->used = s_used;
    if (s_sample < ms) F->status = NAVGPU_ERR_CAPACITY;
  }
}

// The new set's histogram (leaf count), clusters and statistics; then it replaces the filter's set as pf_init leaves it
__global__ __launch_bounds__(kRsThreads) void k_amcl_init_set(AmclDev d, AmclResampleDev r, AmclInitParamsDev p, uint32_t first,
                                                              AmclInitFilterDev* filters) {
  AmclInitFilterDev* F = filters + blockIdx.x;
  if (!F->active || F->status != NAVGPU_OK) return;
  if (p.scored && p.draw_device && F->used > p.max_candidates) {  // device draws: the samples' retries summed
    if (threadIdx.x == 0) F->status = NAVGPU_ERR_CAPACITY;
    return;
  }
  __shared__ int sh[kRsThreads];
  __shared__ int s_bad, s_changed;
  const uint32_t f = first + blockIdx.x;
  const int t = threadIdx.x, nt = blockDim.x, ms = (int)d.max_samples;
  const uint32_t P = r.P;
  const size_t fo = (size_t)f * ms;
  const double* cand = r.cand + fo * 3;
  uint64_t* skey = r.skey + (size_t)f * P;
  uint32_t* sidx = r.sidx + (size_t)f * P;
  if (t == 0) s_bad = 0;
  __syncthreads();
  for (int k = t; k < (int)P; k += nt) {
    uint64_t key = kNoKey;
    if (k < ms && !binKey(cand + 3 * (size_t)k, key)) s_bad = 1;
    skey[k] = key;
    sidx[k] = k < ms ? (uint32_t)k : 0xFFFFFFFFu;
  }
  __syncthreads();
  if (s_bad) {  // a non-finite pose or a bin beyond 2^20 - 2
    if (t == 0) F->status = NAVGPU_ERR_INVALID;
    return;
  }
  bitonicSort(skey, sidx, P);
  const SetWork sw{cand, r.cs + fo * 2, skey, sidx, r.a + (size_t)f * P, r.b + (size_t)f * P, r.label + fo, r.ukey + fo, r.cstart + fo, P};
  const int U = occupiedBins(sw, ms, sh);
  connectComponents(sw, U, &s_changed);
  const int C = numberClusters(sw, ms, sh);
  clusterStats(sw, ms, C, r.cl_count + fo, r.cl_stats + fo * 13, r.set_stats + 12 * (size_t)f);
  for (int i = t; i < ms; i += nt) {
    double* o = d.poses + (fo + i) * 3;
    o[0] = cand[3 * (size_t)i];
    o[1] = cand[3 * (size_t)i + 1];
    o[2] = cand[3 * (size_t)i + 2];
    d.weights[fo + i] = 1.0 / ms;
  }
  if (t == 0) {
    d.w[2 * (size_t)f] = d.w[2 * (size_t)f + 1] = 0.0;
    F->leaf_out = U;
    F->cluster_count = C;
  }
}
}  // namespace

void launch_amcl_init(const AmclDev& d, const AmclResampleDev& r, const AmclInitParamsDev& p, const navgpu_amcl_laser_params& P,
                      const double* beams, int max_n_beams, double2* records, uint32_t first, uint32_t count, AmclInitFilterDev* filters,
                      hipStream_t s) {
  const dim3 lanes((d.max_samples + kInitThreads - 1) / kInitThreads, count);
  const size_t lds = p.scored ? sizeof(double) * 2 * (size_t)max_n_beams : 0;
  if (p.gaussian) {
    if (!p.draw_device) hipLaunchKernelGGL(k_amcl_init_records, dim3(count), dim3(kGaussThreads), 0, s, records, d.max_samples, filters);
    hipLaunchKernelGGL(k_amcl_init_gauss, lanes, dim3(kInitThreads), 0, s, d, r, p, records, first, filters);
  } else if (p.scored && !p.draw_device) {
    hipLaunchKernelGGL(k_amcl_init_chain, dim3(count), dim3(kInitThreads), lds, s, d, r, p, P, beams, first, filters);
  } else {
    hipLaunchKernelGGL(k_amcl_init_free, lanes, dim3(kInitThreads), lds, s, d, r, p, P, beams, first, filters);
  }
  hipLaunchKernelGGL(k_amcl_init_set, dim3(count), dim3(kRsThreads), 0, s, d, r, p, first, filters);
}

}  // namespace navgpu
