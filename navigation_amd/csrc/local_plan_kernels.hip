// k_plan_window: LocalPlannerUtil::getLocalPlan (base_local_planner/src/local_planner_util.cpp:105-123) for robots whose global
// plan lives on the device - transformGlobalPlan's window (goal_functions.cpp:88-174) and prunePlan (:69-86) - and k_plan_scatter
// (navgpu_local_planner_set_plans' upload).  gfx950, wave64.
//
// The reference's loops are restated as first-match searches over the stored plan: a workgroup per robot looks at
// kPlanWindowThreads poses at a time, every wave ballots its lanes' answers and the smallest matching index of the chunk is
// taken across the waves in LDS.  Every comparison sees the same fp64 products and sums as the reference's x86-64 build (the
// file is built with -ffp-contract=off and calls no transcendental: the transform's cos / sin arrive from the host's libm).
// No atomics, nothing shared between workgroups: the result is a function of the inputs alone.
#include <limits.h>

#include "navgpu_device.h"

namespace navgpu {

constexpr int kPwWaves = kPlanWindowThreads / 64;
constexpr int kPwNone = INT_MAX;

// the smallest index base + threadIdx.x of the workgroup whose `hit` is set, kPwNone if there is none; uniform over the workgroup
__device__ __forceinline__ int pwFirstMatch(bool hit, int base, int* wave_first) {
  const unsigned long long m = __ballot(hit);
  if ((threadIdx.x & 63) == 0) wave_first[threadIdx.x >> 6] = m ? base + (int)threadIdx.x + __ffsll((long long)m) - 1 : kPwNone;
  __syncthreads();
  int r = kPwNone;
#pragma unroll
  for (int w = 0; w < kPwWaves; ++w) r = min(r, wave_first[w]);
  __syncthreads();  // (wave_first is written again by the next chunk)
  return r;
}

struct PwPoint {
  double x, y;
};
// a stored pose in the global frame (goal_functions.cpp:148-150 with a planar transform); the stored values without one
__device__ __forceinline__ PwPoint pwToGlobal(const PlanWindowIn& a, double px, double py) {
  if (!(a.flags & kPwTransform)) return PwPoint{px, py};
  return PwPoint{a.c * px - a.sn * py + a.tx, a.sn * px + a.c * py + a.ty};
}

__global__ __launch_bounds__(kPlanWindowThreads) void k_plan_window(PlannerDev pl, const navgpu_global_pose* store, uint32_t max_global_plan,
                                                                    uint32_t first, const PlanWindowIn* in, PlanWindowRec* rec, double sq_thr) {
  __shared__ int wave_first[kPwWaves];
  const uint32_t inst = first + blockIdx.x;
  const PlanWindowIn a = in[inst];
  if (!(a.flags & kPwActive)) return;  // (the whole workgroup: robots of the range that are not resident, have no pose or no plan)
  const navgpu_global_pose* p = store + (size_t)inst * max_global_plan + a.start;
  const int n = (int)a.len, tid = (int)threadIdx.x, max_plan = (int)pl.max_plan;
  PlanWindowRec out{};
  out.w.first_index = -1;
  out.w.remaining = n;
  out.w.status = NAVGPU_LOCAL_WINDOW_OK;
  // getGoalPose (goal_functions.cpp:175-214): the last stored pose in the global frame (the erase below never takes it unless it
  // takes every pose)
  {
    const navgpu_global_pose g = p[n - 1];
    const PwPoint gg = pwToGlobal(a, g.x, g.y);
    out.goal[0] = gg.x;
    out.goal[1] = gg.y;
    out.goal[2] = (a.flags & kPwTransform) ? g.yaw + a.tyaw : g.yaw;
  }
  // 1. i0: the first stored pose within reach (:126-134).  A NaN coordinate fails <= and is passed over.
  int i0 = kPwNone;
  for (int base = 0; base < n && i0 == kPwNone; base += (int)kPlanWindowThreads) {
    const int i = base + tid;
    bool hit = false;
    if (i < n) {
      const double xd = a.robot[0] - p[i].x, yd = a.robot[1] - p[i].y;
      hit = xd * xd + yd * yd <= sq_thr;
    }
    i0 = pwFirstMatch(hit, base, wave_first);
  }
  if (i0 == kPwNone) {  // "Received an empty transformed plan.": nothing is emitted, the robot's window of the cycle before stays
    if (tid == 0) rec[inst] = out;
    return;
  }
  // 2. j: the first pose behind i0 that is out of reach, or NaN; it is still taken (:140-154).  Looked for among the max_plan poses
  //    a window may hold: if they are all within reach and the plan goes on, the window does not fit.
  const int hi = (int)min((long long)n, (long long)i0 + max_plan);  // (n <= INT_MAX: navgpu_local_planner_reserve_plans)
  int j = kPwNone;
  for (int base = i0 + 1; base < hi && j == kPwNone; base += (int)kPlanWindowThreads) {
    const int i = base + tid;
    bool hit = false;
    if (i < hi) {
      const double xd = a.robot[0] - p[i].x, yd = a.robot[1] - p[i].y;
      hit = !(xd * xd + yd * yd <= sq_thr);
    }
    j = pwFirstMatch(hit, base, wave_first);
  }
  if (j == kPwNone) {
    if ((long long)i0 + max_plan < (long long)n) {  // 3. more than max_plan poses: nothing is pruned, nothing emitted
      if (tid == 0) {
        out.w.first_index = i0;
        out.w.status = NAVGPU_LOCAL_WINDOW_CAPACITY;
        rec[inst] = out;
      }
      return;
    }
    j = n - 1;  // the window runs to the end of the plan
  }
  const int m = j - i0 + 1;
  // 4. prunePlan: e leading window poses are erased, up to the first whose transformed point is closer than 1 m to the robot
  int e = 0;
  if (a.flags & kPwPrune) {
    e = kPwNone;
    for (int base = 0; base < m && e == kPwNone; base += (int)kPlanWindowThreads) {
      const int q = base + tid;
      bool hit = false;
      if (q < m) {
        const PwPoint g = pwToGlobal(a, p[i0 + q].x, p[i0 + q].y);
        const double xd = a.pose[0] - g.x, yd = a.pose[1] - g.y;
        hit = xd * xd + yd * yd < 1;
      }
      e = pwFirstMatch(hit, base, wave_first);
    }
    if (e == kPwNone) e = m;
  }
  // 5. the local plan: window positions [e, m) as x, y pairs (what updatePlanAndLocalCosts takes)
  double* dst = pl.plan + (size_t)inst * pl.max_plan * 2;
  for (int q = e + tid; q < m; q += (int)kPlanWindowThreads) {
    const PwPoint g = pwToGlobal(a, p[i0 + q].x, p[i0 + q].y);
    dst[2 * (q - e)] = g.x;
    dst[2 * (q - e) + 1] = g.y;
  }
  // 6. the record.  The erase is from the FRONT of the stored plan (global_it = global_plan.begin(), :73), whatever i0 is.
  if (tid == 0) {
    if (m > e) pl.plan_count[inst] = (uint32_t)(m - e);  // (an empty local plan leaves window and count as they were: nothing is staged then)
    out.w.first_index = i0;
    out.w.n_window = m;
    out.w.n_erased = e;
    out.w.n_local = m - e;
    out.w.remaining = n - e;
    if (m > e) {
      const PwPoint g = pwToGlobal(a, p[i0 + m - 1].x, p[i0 + m - 1].y);
      out.last[0] = g.x;
      out.last[1] = g.y;
    }
    rec[inst] = out;
  }
}

// One workgroup per plan; lanes stride over its doubles, so loads and stores are coalesced.
__global__ __launch_bounds__(256) void k_plan_scatter(const navgpu_global_pose* poses, const uint32_t* offsets, navgpu_global_pose* slots,
                                                      uint32_t max_global_plan) {
  const uint32_t at = offsets[blockIdx.x], len = min(offsets[blockIdx.x + 1] - at, max_global_plan);
  const double* src = reinterpret_cast<const double*>(poses + at);
  double* dst = reinterpret_cast<double*>(slots + (size_t)blockIdx.x * max_global_plan);
  for (size_t i = threadIdx.x; i < 3 * (size_t)len; i += 256) dst[i] = src[i];
}

void launch_plan_window(const PlannerDev& pl, const navgpu_global_pose* store, uint32_t max_global_plan, uint32_t first, uint32_t count,
                        const PlanWindowIn* in, PlanWindowRec* rec, double sq_dist_threshold, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_window, dim3(count), dim3(kPlanWindowThreads), 0, s, pl, store, max_global_plan, first, in, rec, sq_dist_threshold);
}
void launch_plan_scatter(const navgpu_global_pose* poses, const uint32_t* offsets, uint32_t count, navgpu_global_pose* slots,
                         uint32_t max_global_plan, hipStream_t s) {
  hipLaunchKernelGGL(k_plan_scatter, dim3(count), dim3(256), 0, s, poses, offsets, slots, max_global_plan);
}

}  // namespace navgpu
