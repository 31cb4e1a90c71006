// The workgroup scan the order-preserving compactions share (voxel_export_kernels.hip, obs_buffer_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace navgpu {

constexpr uint32_t kScanThreads = 256;  // lanes of a scanning workgroup

// Exclusive prefix of v over the workgroup's lanes in lane order, and the workgroup's total.  Inside a wave a Hillis-Steele
// scan on __shfl_up (6 steps for 64 lanes), across the 4 waves their totals through LDS.  Every lane of the kScanThreads
// calls it (two barriers); s_wave holds kScanThreads / 64 words.
__device__ __forceinline__ uint32_t blockExclusive(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
    const uint32_t t = s_wave[w];
    before += w < wave ? t : 0u;
    total += t;
  }
  __syncthreads();  // s_wave may be written again
  return before + inc - v;
}

}  // namespace navgpu
