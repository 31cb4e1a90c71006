// drand48() on the device: the 48-bit LCG (a = 0x5DEECE66D, c = 0xB) with jump-ahead, and pf_ran_gaussian's polar Box-Muller
// rejection loop (pf/pf_pdf.c:132-146) as a stream compaction.  Shared by the motion model (amcl_motion_kernels.hip) and the
// Gaussian / uniform init (amcl_init_kernels.hip).
// pf_ran_gaussian's rejection loop consumes a data-dependent but fully determined number of drand48() values: values equal to 0.0
// are skipped, the others pair up consecutively as (x1, x2), and a pair is accepted when 0 < w = x1*x1 + x2*x2 <= 1 (exact IEEE
// arithmetic).  Lanes generate the stream in rounds by LCG jump-ahead, the nonzero values are scanned into a compacted list, the
// pairs are tested, and the accepted pairs are scanned into record indices.  A record is (x2, sqrt(-2.0*log(w)/w)) rather than a
// unit deviate because the reference multiplies sigma * x2 first.
#pragma once
#include <hip/hip_runtime.h>

#include "navgpu_amcl.h"

namespace navgpu {
namespace {
constexpr int kGaussThreads = 256;
constexpr int kGaussWaves = kGaussThreads / 64;
constexpr int kPerLane = 8;                                      // drand48 values per lane per round
constexpr int kRound = kGaussThreads * kPerLane;                 // values per round
constexpr int kPairsPerLane = (kRound + 1 + 2 * kGaussThreads - 1) / (2 * kGaussThreads);  // pairs of a round (with the carry)
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

// `need` records (pf_ran_gaussian deviates, need >= 1) from the drand48 state *state in the reference's draw order, into rec; every
// thread of a kGaussThreads workgroup calls it.  *state comes back advanced past the last value used.
__device__ void drand48GaussRecords(double2* rec, int need, uint64_t* state) {
  __shared__ uint64_t sv[kRound + 2];  // the round's nonzero values as LCG states, after the carried one
  __shared__ int wsum[kGaussWaves];
  __shared__ uint64_t s_x, s_next, s_carry_state, s_final;
  __shared__ int s_carry, s_rec;
  const int t = threadIdx.x;
  const Affine lane_jump = jump((uint32_t)(t * kPerLane));
  if (t == 0) {
    s_x = *state;
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
  if (t == 0) *state = s_final;
}

}  // namespace
}  // namespace navgpu
