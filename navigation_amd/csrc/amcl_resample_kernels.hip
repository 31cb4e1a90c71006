// amcl's resampling step on the device, for a batch of particle filters (one workgroup per filter).
//   pf_update_resample (amcl/src/amcl/pf/pf.c:512-562)
//     pf_resample_multinomial (:408-510), pf_resample_systematic (:319-405), pf_resample_limit (:567-588)
//     pf_kdtree_insert's histogram (pf_kdtree.c:110-120): a sort of packed bin keys, not a tree
//     pf_cluster_stats (:592-720) with pf_kdtree_cluster (pf_kdtree.c:358-437): label propagation over the occupied bins
//     pf_update_converged (:222-253)
// Every decision the reference makes from a floating-point value uses the reference's own expression in fp64 (the library is built
// with -ffp-contract=off): the cumulative table c[i+1] = c[i] + w[i] in sample order, the systematic targets
// target += delta; if (target > 1.0) target = 0.0, the KLD limit.  Sums are sequential in sample order (the reference's own
// order) in one lane per cluster, so two runs give the same bytes; no floating-point atomics.  The per-filter workspace
// (AmclResampleDev) is global memory: every phase is a loop of the workgroup's threads separated by __syncthreads, or a
// sequential loop of one lane where the reference's order decides the result.
#include <hip/hip_runtime.h>

#include "amcl_pf_stages.h"

namespace navgpu {

namespace {
constexpr uint32_t kStartDraw = 0xFFFFFFFFu;  // draw index of systematic_sample_start (device draws)

// pf_resample_limit (pf.c:567-588); n above max_samples (where the reference's int conversion could overflow) is max_samples
__device__ int kldLimit(const AmclResampleParamsDev& p, int k) {
  if (k <= 1) return p.max_samples;
  const double a = 1;
  const double b = 2 / (9 * ((double)k - 1));
  const double c = sqrt(2 / (9 * ((double)k - 1))) * p.pop_z;
  const double x = a - b + c;
  const double n = ceil((k - 1) / (2 * p.pop_err) * x * x * x);
  if (n < p.min_samples) return p.min_samples;
  if (!(n <= p.max_samples)) return p.max_samples;
  return (int)n;
}

// The sample whose interval [c[i], c[i+1]) holds r (the reference's linear scan, pf.c:376-386, 474-479), by binary search over the
// non-decreasing table.  Where no interval holds r (r < 0, r >= c[n], NaN) the reference loops forever or reads samples[n]: here
// the last sample with positive weight (`fallback`).
__device__ __forceinline__ int pickIndex(const double* c, int n, double r, int fallback) {
  if (!(r >= 0.0 && r < c[n])) return fallback;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid + 1] > r)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kRsThreads) void k_amcl_resample(AmclDev d, AmclResampleDev r, AmclResampleParamsDev p, uint32_t first,
                                                              AmclResampleFilterDev* filters) {
  AmclResampleFilterDev* F = filters + blockIdx.x;
  if (!F->active) return;
  __shared__ int sh[kRsThreads];
  __shared__ int s_err, s_M, s_nrand, s_fallback, s_bad, s_count, s_leaf, s_changed, s_conv;
  __shared__ double s_mx, s_my;
  const uint32_t f = first + blockIdx.x;
  const int t = threadIdx.x, nt = blockDim.x, ms = p.max_samples, n = F->sample_count;
  const uint32_t P = r.P;
  const size_t fo = (size_t)f * ms;
  const double* w_in = d.weights + fo;
  double* c = r.c + (size_t)f * (ms + 1);
  double* cand = r.cand + fo * 3;
  double* cs = r.cs + fo * 2;  // systematic targets first, cos / sin of set b later
  uint64_t* skey = r.skey + (size_t)f * P;
  uint32_t* sidx = r.sidx + (size_t)f * P;
  int* a = r.a + (size_t)f * P;
  int* b = r.b + (size_t)f * P;
  int* label = r.label + fo;
  uint64_t* ukey = r.ukey + fo;
  int* cstart = r.cstart + fo;
  const AmclMapDev& map = d.maps[f];
  const bool sys = p.model == NAVGPU_AMCL_RESAMPLE_SYSTEMATIC, dev = p.draw_device != 0;
  const uint64_t call = F->rng_ctr;
  // pf_update_resample (pf.c:526-528); w_slow = 0 gives NaN (0 / 0) or -inf: taken as 0, as the multinomial draw `u < NaN` does
  double w_diff = 1.0 - d.w[2 * (size_t)f + 1] / d.w[2 * (size_t)f];
  if (w_diff < 0.0) w_diff = 0.0;
  if (w_diff != w_diff) w_diff = 0.0;

  // 1. cumulative table in sample order; systematic: new_count, n_rand and the target sequence (pf.c:330-388)
  if (t == 0) {
    int err = n <= 0, fallback = n - 1, M = ms, nrand = 0;
    double acc = 0.0;
    c[0] = 0.0;
    for (int i = 0; i < n; ++i) {
      const double w = w_in[i];
      acc = acc + w;
      c[i + 1] = acc;
      if (w > 0) fallback = i;
    }
    if (sys) {
      int new_count = kldLimit(p, F->leaf_in);
      if (w_diff > 0.0) {
        new_count = (int)(new_count * (1.0 + w_diff));
        if (new_count > ms) new_count = ms;
      }
      nrand = (int)(w_diff * new_count);
      const int nsys = new_count - nrand;
      double start = F->sys_start, u1;
      if (dev) draw2(p.seed, f, call, kStartDraw, 0, start, u1);
      if (nsys > 0) {  // nsys == 0 (w_diff == 1): every sample is random and delta = 1 / 0 is never used
        const double delta = 1.0 / nsys;
        double target = start;
        for (int j = 0; j < nsys; ++j) {
          cs[j] = target;
          target += delta;
          if (target > 1.0) target = 0.0;
        }
      }
      if (!dev && nrand > F->pool_count) err = 1;
      M = new_count;
    }
    s_err = err;
    s_M = M;
    s_nrand = nrand;
    s_fallback = fallback;
    s_bad = M;
  }
  __syncthreads();
  if (s_err) {
    if (t == 0) F->status = NAVGPU_ERR_INVALID;
    return;
  }
  const int M = s_M, nrand = s_nrand, fallback = s_fallback;

  // 2. multinomial: which candidates are random, and each one's rank in the random-pose source
  if (!sys) {
    for (int k = t; k < M; k += nt) {
      double uf, up;
      if (dev)
        draw2(p.seed, f, call, k, 0, uf, up);
      else
        uf = r.u[(blockIdx.x * (size_t)ms + k) * 2];
      a[k] = uf < w_diff;
    }
    __syncthreads();
    blockScan(a, M, sh);
  }

  // 3. candidate poses and their bin keys
  const double* pool = dev ? nullptr : r.pool + 3 * F->pool_off;
  for (int k = t; k < (int)P; k += nt) {
    if (k >= M) {
      skey[k] = kNoKey;
      sidx[k] = 0xFFFFFFFFu;
      continue;
    }
    double pose[3] = {0.0, 0.0, 0.0};
    bool random, ok = true;
    int q = k, src = 0;
    if (sys) {
      random = k < nrand;
      if (!random) src = pickIndex(c, n, cs[k - nrand], fallback);
    } else {
      double uf, up;
      if (dev)
        draw2(p.seed, f, call, k, 0, uf, up);
      else {
        uf = r.u[(blockIdx.x * (size_t)ms + k) * 2];
        up = r.u[(blockIdx.x * (size_t)ms + k) * 2 + 1];
      }
      random = uf < w_diff;
      if (random)
        q = a[k];
      else
        src = pickIndex(c, n, up, fallback);
    }
    if (random) {
      if (dev) {
        double uc, ut;
        draw2(p.seed, f, call, k, 1, uc, ut);
        ok = freePose(map, uc, ut, pose);
      } else if (q < F->pool_count) {
        pose[0] = pool[3 * (size_t)q];
        pose[1] = pool[3 * (size_t)q + 1];
        pose[2] = pool[3 * (size_t)q + 2];
      } else {
        ok = false;
      }
    } else {
      const double* s = d.poses + (fo + src) * 3;
      pose[0] = s[0];
      pose[1] = s[1];
      pose[2] = s[2];
    }
    uint64_t key = kNoKey;
    if (ok) ok = binKey(pose, key);
    cand[3 * (size_t)k] = pose[0];
    cand[3 * (size_t)k + 1] = pose[1];
    cand[3 * (size_t)k + 2] = pose[2];
    skey[k] = ok ? key : kNoKey;
    sidx[k] = (uint32_t)k;
    label[k] = random;
    if (!ok) atomicMin(&s_bad, k);
  }
  __syncthreads();

  // 4. histogram: first occurrence of every bin among the candidates
  bitonicSort(skey, sidx, P);
  for (int k = t; k < M; k += nt) a[k] = 0;
  __syncthreads();
  for (int q = t; q < M; q += nt)
    if (skey[q] != kNoKey && (q == 0 || skey[q] != skey[q - 1])) a[sidx[q]] = 1;
  __syncthreads();

  // 5. multinomial: the reference stops after candidate k (1-based) once k > pf_resample_limit(leaf_count(k)) (pf.c:503-504)
  if (t == 0) {
    int leaf = 0, count = M, lim_leaf = -1, lim = 0, err = 0, rnd = 0;
    for (int k = 0; k < M; ++k) {
      if (k >= s_bad) {  // a candidate without a pose (pool exhausted, no free cell) or with a bin outside the key range
        err = 1;
        break;
      }
      leaf += a[k];
      rnd += label[k];
      if (!sys) {
        if (leaf != lim_leaf) {
          lim = kldLimit(p, leaf);
          lim_leaf = leaf;
        }
        if (k + 1 > lim) {
          count = k + 1;
          break;
        }
      }
    }
    s_err = err;
    s_count = count;
    s_leaf = leaf;
    F->n_random = rnd;
  }
  __syncthreads();
  if (s_err) {
    if (t == 0) F->status = NAVGPU_ERR_INVALID;
    return;
  }
  const int count = s_count;

  // 6-9. occupied bins of set b, their components, the clusters and their statistics (amcl_pf_stages.h)
  const SetWork sw{cand, cs, skey, sidx, a, b, label, ukey, cstart, P};
  const int U = occupiedBins(sw, count, sh);
  connectComponents(sw, U, &s_changed);
  const int C = numberClusters(sw, count, sh);
  clusterStats(sw, count, C, r.cl_count + fo, r.cl_stats + fo * 13, r.set_stats + 12 * (size_t)f);
  const double total = (double)count;
  if (t == 64) {  // pf_update_converged's means (pf.c:230-240), in another wave
    double mx = 0, my = 0;
    for (int i = 0; i < count; ++i) {
      mx += cand[3 * (size_t)i];
      my += cand[3 * (size_t)i + 1];
    }
    mx /= count;
    my /= count;
    s_mx = mx;
    s_my = my;
    s_conv = 1;
  }
  __syncthreads();

  // 10. pf_update_converged's test, then set b replaces set a (pf.c:541-556)
  const double mx = s_mx, my = s_my;
  for (int i = t; i < count; i += nt) {
    if (fabs(cand[3 * (size_t)i] - mx) > p.dist_threshold || fabs(cand[3 * (size_t)i + 1] - my) > p.dist_threshold) s_conv = 0;
    double* o = d.poses + (fo + i) * 3;
    o[0] = cand[3 * (size_t)i];
    o[1] = cand[3 * (size_t)i + 1];
    o[2] = cand[3 * (size_t)i + 2];
    d.weights[fo + i] = 1.0 / total;
  }
  __syncthreads();
  if (t == 0) {
    if (w_diff > 0.0) d.w[2 * (size_t)f] = d.w[2 * (size_t)f + 1] = 0.0;
    F->status = NAVGPU_OK;
    F->count = count;
    F->leaf_out = s_leaf;
    F->converged = s_conv;
    F->cluster_count = C;
  }
}
}  // namespace

void launch_amcl_resample(const AmclDev& d, const AmclResampleDev& r, const AmclResampleParamsDev& p, uint32_t first, uint32_t count,
                          AmclResampleFilterDev* filters, hipStream_t s) {
  hipLaunchKernelGGL(k_amcl_resample, dim3(count), dim3(kRsThreads), 0, s, d, r, p, first, filters);
}

}  // namespace navgpu
