// Stages of the particle set's histogram and cluster statistics, shared by k_amcl_resample (amcl_resample_kernels.hip) and the
// init kernels (amcl_init_kernels.hip).  Every stage is called by all threads of one workgroup per filter, over that filter's
// slice of AmclResampleDev.
//   binKey / bitonicSort:  pf_kdtree_insert's histogram (pf_kdtree.c:110-120), a sort of packed bin keys, not a tree
//   occupiedBins:          the occupied bins, ascending, and each sample's bin
//   connectComponents:     pf_kdtree_cluster (pf_kdtree.c:358-437) as label propagation over the occupied bins
//   numberClusters:        clusters numbered by their lowest sample index
//   clusterStats:          pf_cluster_stats (pf.c:592-720), summed in sample order in one lane per cluster
#pragma once
#include <hip/hip_runtime.h>

#include "navgpu_amcl.h"

namespace navgpu {
namespace {
constexpr int kRsThreads = 1024;
constexpr int kKeyBits = 21;
constexpr int64_t kKeyBias = 1 << 20;
constexpr double kKeyLimit = (double)(kKeyBias - 2);  // |bin| <= 2^20 - 2: the +-1 neighbours of a bin stay inside its field
constexpr uint64_t kNoKey = ~0ull;

// AmclNode::randomFreeSpacePose (amcl_node.cpp:1200-1212) with u_cell, u_theta in place of its two drand48() calls
__device__ bool freePose(const AmclMapDev& m, double u_cell, double u_theta, double* out) {
  if (m.n_free <= 0 || !m.free_cells) return false;
  const unsigned idx = (unsigned)(u_cell * (double)m.n_free);
  if (idx >= (unsigned)m.n_free) return false;
  const int cell = m.free_cells[idx], i = cell % m.sx, j = cell / m.sx;
  out[0] = m.ox + (i - m.sx / 2) * m.scale;  // MAP_WXGX / MAP_WYGY (map.h:133-134)
  out[1] = m.oy + (j - m.sy / 2) * m.scale;
  out[2] = u_theta * 2 * M_PI - M_PI;
  return true;
}

// pf_kdtree_insert's key (pf_kdtree.c:116-118) packed as three biased 21-bit fields; false for a non-finite pose or |bin| > 2^20 - 2
__device__ __forceinline__ bool binKey(const double* pose, uint64_t& key) {
  const double size[3] = {0.50, 0.50, (10 * M_PI / 180)};
  uint64_t k = 0;
  for (int a = 0; a < 3; ++a) {
    const double b = floor(pose[a] / size[a]);
    if (!(b >= -kKeyLimit && b <= kKeyLimit)) return false;
    k = (k << kKeyBits) | (uint64_t)((int64_t)b + kKeyBias);
  }
  key = k;
  return true;
}

__device__ __forceinline__ int findKey(const uint64_t* keys, int n, uint64_t k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && keys[lo] == k ? lo : -1;
}

// exclusive prefix sum of a[0, n) in place; every thread of the workgroup calls it; returns the total
__device__ int blockScan(int* a, int n, int* sh) {
  int carry = 0;
  const int t = threadIdx.x, nt = blockDim.x;
  for (int base = 0; base < n; base += nt) {
    const int i = base + t;
    const int v = i < n ? a[i] : 0;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {
      const int x = t >= off ? sh[t - off] : 0;
      __syncthreads();
      sh[t] += x;
      __syncthreads();
    }
    if (i < n) a[i] = carry + sh[t] - v;
    carry += sh[nt - 1];
    __syncthreads();
  }
  return carry;
}

// ascending bitonic sort of the pairs (key, idx) over P (a power of two) slots
__device__ void bitonicSort(uint64_t* key, uint32_t* idx, uint32_t P) {
  for (uint32_t k = 2; k <= P; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint64_t ki = key[i], kl = key[l];
          const uint32_t ii = idx[i], il = idx[l];
          const bool gt = ki > kl || (ki == kl && ii > il);
          if (gt == ((i & k) == 0)) {
            key[i] = kl;
            key[l] = ki;
            idx[i] = il;
            idx[l] = ii;
          }
        }
      }
      __syncthreads();
    }
}

// One filter's set and workspace
struct SetWork {
  const double* pose;  // [count][3] the set's poses
  double* cs;          // [count][2] cos, sin of the angles (written by numberClusters)
  uint64_t* skey;      // [P] the set's bin keys, sorted (in); cluster keys (numberClusters)
  uint32_t* sidx;      // [P] sample index of each sorted key
  int* a;
  int* b;              // each sample's bin
  int* label;          // each bin's component label
  uint64_t* ukey;      // occupied bins, ascending
  int* cstart;         // first position of each cluster in the second sort
  uint32_t P;
};

// occupied bins of the set's first `count` samples (runs of the sorted keys whose first sample is < count), ascending, and each
// sample's bin; returns their number
__device__ int occupiedBins(const SetWork& w, int count, int* sh) {
  const int t = threadIdx.x, nt = blockDim.x;
  const uint32_t P = w.P;
  uint64_t* skey = w.skey;
  uint32_t* sidx = w.sidx;
  int *a = w.a, *b = w.b, *label = w.label;
  uint64_t* ukey = w.ukey;
  for (int q = t; q < (int)P; q += nt)
    a[q] = skey[q] != kNoKey && (int)sidx[q] < count && (q == 0 || skey[q] != skey[q - 1]);
  __syncthreads();
  const int U = blockScan(a, P, sh);
  for (int q = t; q < (int)P; q += nt) {
    if (skey[q] == kNoKey || (int)sidx[q] >= count) continue;
    const bool start = q == 0 || skey[q] != skey[q - 1];
    const int u = start ? a[q] : a[q] - 1;
    b[sidx[q]] = u;
    if (start) {
      ukey[u] = skey[q];
      label[u] = (int)sidx[q];
    }
  }
  __syncthreads();

  return U;
}

// connected components over the 26-neighbourhood, no angular wrap (pf_kdtree.c:407-437): every bin takes the smallest label of
// its neighbours and of its label's own bin until nothing changes; the fixed point is the component's lowest sample index
__device__ void connectComponents(const SetWork& w, int U, int* s_changed) {
  const int t = threadIdx.x, nt = blockDim.x;
  const int *b = w.b;
  int* label = w.label;
  const uint64_t* ukey = w.ukey;
  for (;;) {
    if (t == 0) *s_changed = 0;
    __syncthreads();
    for (int u = t; u < U; u += nt) {
      const uint64_t key = ukey[u];
      int l = label[u];
      for (int o = 0; o < 27; ++o) {
        if (o == 13) continue;
        const int64_t dx = o / 9 - 1, dy = (o % 9) / 3 - 1, dt = o % 3 - 1;
        const uint64_t nk = key + (uint64_t)((dx << (2 * kKeyBits)) + (dy << kKeyBits) + dt);
        const int v = findKey(ukey, U, nk);
        if (v >= 0) l = min(l, label[v]);
      }
      l = min(l, label[b[l]]);
      if (l < label[u]) {
        label[u] = l;
        *s_changed = 1;
      }
    }
    __syncthreads();
    if (!*s_changed) break;
    __syncthreads();
  }

}

// clusters numbered by their lowest sample index, samples sorted by cluster; cos / sin of every angle.  Returns their number.
__device__ int numberClusters(const SetWork& w, int count, int* sh) {
  const int t = threadIdx.x, nt = blockDim.x;
  const uint32_t P = w.P;
  const double* cand = w.pose;
  double* cs = w.cs;
  uint64_t* skey = w.skey;
  uint32_t* sidx = w.sidx;
  int *a = w.a, *b = w.b, *label = w.label, *cstart = w.cstart;
  for (int i = t; i < count; i += nt) {
    a[i] = label[b[i]] == i;
    cs[2 * (size_t)i] = cos(cand[3 * (size_t)i + 2]);
    cs[2 * (size_t)i + 1] = sin(cand[3 * (size_t)i + 2]);
  }
  __syncthreads();
  const int C = blockScan(a, count, sh);
  for (int q = t; q < (int)P; q += nt) {
    if (q < count) {
      skey[q] = (uint64_t)a[label[b[q]]];
      sidx[q] = (uint32_t)q;
    } else {
      skey[q] = kNoKey;
      sidx[q] = 0xFFFFFFFFu;
    }
  }
  __syncthreads();
  bitonicSort(skey, sidx, P);
  for (int q = t; q < count; q += nt)
    if (q == 0 || skey[q] != skey[q - 1]) cstart[skey[q]] = q;
  __syncthreads();

  return C;
}

// pf_cluster_stats (pf.c:592-720): per cluster in one lane, summed in sample order; the set's statistics in lane 0
__device__ void clusterStats(const SetWork& sw, int count, int C, int* cl_count, double* cl, double* set_stats) {
  const int t = threadIdx.x, nt = blockDim.x;
  const double* cand = sw.pose;
  const double* cs = sw.cs;
  const uint32_t* sidx = sw.sidx;
  const int* cstart = sw.cstart;
  const double total = (double)count, w = 1.0 / total;
  for (int k = t; k < C; k += nt) {
    const int s = cstart[k], e = k + 1 < C ? cstart[k + 1] : count;
    double weight = 0.0, m[4] = {0.0, 0.0, 0.0, 0.0}, cc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int q = s; q < e; ++q) {
      const size_t i = sidx[q];
      const double v[2] = {cand[3 * i], cand[3 * i + 1]};
      weight += w;
      m[0] += w * v[0];
      m[1] += w * v[1];
      m[2] += w * cs[2 * i];
      m[3] += w * cs[2 * i + 1];
      for (int j = 0; j < 2; j++)
        for (int l = 0; l < 2; l++) cc[j][l] += w * v[j] * v[l];
    }
    double* o = cl + 13 * (size_t)k;
    const double mean[3] = {m[0] / weight, m[1] / weight, atan2(m[3], m[2])};
    o[0] = weight;
    o[1] = mean[0];
    o[2] = mean[1];
    o[3] = mean[2];
    for (int j = 0; j < 9; ++j) o[4 + j] = 0.0;
    for (int j = 0; j < 2; j++)
      for (int l = 0; l < 2; l++) o[4 + 3 * j + l] = cc[j][l] / weight - mean[j] * mean[l];
    o[4 + 8] = -2 * log(sqrt(m[2] * m[2] + m[3] * m[3]));
    cl_count[k] = e - s;
  }
  if (t == 0) {  // the set's statistics
    double weight = 0.0, m[4] = {0.0, 0.0, 0.0, 0.0}, cc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int i = 0; i < count; ++i) {
      const double v[2] = {cand[3 * (size_t)i], cand[3 * (size_t)i + 1]};
      weight += w;
      m[0] += w * v[0];
      m[1] += w * v[1];
      m[2] += w * cs[2 * (size_t)i];
      m[3] += w * cs[2 * (size_t)i + 1];
      for (int j = 0; j < 2; j++)
        for (int l = 0; l < 2; l++) cc[j][l] += w * v[j] * v[l];
    }
    double* o = set_stats;
    const double mean[3] = {m[0] / weight, m[1] / weight, atan2(m[3], m[2])};
    for (int j = 0; j < 3; ++j) o[j] = mean[j];
    for (int j = 0; j < 9; ++j) o[3 + j] = 0.0;
    for (int j = 0; j < 2; j++)
      for (int l = 0; l < 2; l++) o[3 + 3 * j + l] = cc[j][l] / weight - mean[j] * mean[l];
    o[3 + 8] = -2 * log(sqrt(m[2] * m[2] + m[3] * m[3]));
  }
}
}  // namespace
}  // namespace navgpu
