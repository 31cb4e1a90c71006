// The trajectory cloud of DWAPlanner::findBestPath (dwa_planner.cpp:318-348) from the terms an enabled robot's cycle kept
// (k_score_terms, planner_score.hip): k_traj_scan replays SimpleScoredSamplingPlanner's early-out flow as scans over the sample
// slots, k_traj_emit rolls the member slots' trajectories and writes the points (gfx950).  Both run at the read call
// (navgpu_traj_cloud.cpp), not in the cycle.  Compiled with -ffp-contract=off like the scorer: the sums are addCritic's, in its order.
#include "planner_score.h"

namespace navgpu {

// ------------------------------------------------------------------------------------------------
// k_traj_scan: one workgroup for the robot, the slots in chunks of a lane each, state carried from chunk to chunk.
//   (a) the incumbent slot i was scored against (findBestTrajectory, simple_scored_sampling_planner.cpp:111-127):
//         best_i = min { full_j : j < i, slot j scored, full_j >= 0 }, -1 when there is none
//       an EXCLUSIVE PREFIX MINIMUM of the full costs: a slot that early-outs is worse than the incumbent and never becomes
//       it, a slot that does not has cost_ref = full, and the terms are non-negative.
//   (b) cost_ref_i = scoreTrajectory(traj_i, best_i) (:50-79) from the slot's terms: critics with scale 0 skipped, a term of
//       0 not scaled, the sum cut at the first failing critic (its code is the result) or behind the first add that makes
//       best_i > 0 && partial > best_i true.
//   (c) membership (cost >= 0) and the exclusive prefix sum of the members' point counts: a slot's offset in the cloud.
// reference_costs = 0: the cost is the full sum (membership full >= 0).  Wave scans with __shfl_up, one LDS word per wave for
// the carry, no atomics: two calls give identical bytes.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kTrajScanThreads = 256;
constexpr uint32_t kTrajEmitThreads = 256;
constexpr uint32_t kTrajPointFloats = 7;  // base_local_planner::MapGridCostPoint

__global__ __launch_bounds__(kTrajScanThreads) void k_traj_scan(PlannerDev pl, TrajCloudDev t, uint32_t inst) {
  __shared__ double s_min[kTrajScanThreads / 64];
  __shared__ uint32_t s_sum[kTrajScanThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = pl.axis_count[4 * inst + 3];
  const double kNone = 1.0e300;  // no valid slot so far (as the scorer's argmin)
  double carry_min = kNone;
  uint32_t carry_pts = 0;
  for (int base = 0; base < n; base += (int)kTrajScanThreads) {
    const int i = base + (int)tid;
    const bool in = i < n;
    SampleTerms rec = {{0, 0, 0, 0, 0}, 6, 0, NAVGPU_SAMPLE_REJECTED, 0};
    if (in) rec = t.terms[i];
    const bool scored = rec.status == NAVGPU_SAMPLE_SCORED;
    // the full sum, as scoreSamples forms it
    double full = -1.0;
    if (scored) {
      if (rec.first_fail < 6) {
        full = rec.fail_code;
      } else {
        full = 0.0;
        for (int k = 0; k < 5; ++k) addCritic(full, t.scale[k] != 0, rec.v[k], t.scale[k]);
      }
    }
    // ---- (a)
    double incl = (scored && full >= 0.0) ? full : kNone;
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(incl, off);
      if ((int)lane >= off) incl = fmin(incl, o);
    }
    double best = __shfl_up(incl, 1);
    if (lane == 0) best = kNone;
    if (lane == 63) s_min[wave] = incl;
    __syncthreads();
    best = fmin(best, carry_min);
    for (uint32_t w = 0; w < kTrajScanThreads / 64; ++w) {
      const double v = s_min[w];
      if (w < wave) best = fmin(best, v);
      carry_min = fmin(carry_min, v);
    }
    if (best == kNone) best = -1.0;
    // ---- (b)
    double ref = -1.0;
    if (scored) {
      if (rec.first_fail == 0) {  // the oscillation critic (scale 1, never off): its term is 0 or the sample fails
        ref = rec.fail_code;
      } else {
        ref = 0.0;
        for (int k = 0; k < 5; ++k) {
          if (t.scale[k] == 0) continue;
          if (k + 1 == rec.first_fail) {
            ref = rec.fail_code;
            break;
          }
          addCritic(ref, true, rec.v[k], t.scale[k]);
          if (best > 0 && ref > best) break;
        }
      }
    }
    // ---- (c)
    const double cost = t.reference_costs ? ref : full;
    const bool member = scored && cost >= 0.0;
    uint32_t chunk_pts;
    const uint32_t off = carry_pts + blockExclusiveScan1024(member ? (uint32_t)rec.n_points : 0u, s_sum, &chunk_pts);  // (two barriers: s_min is free again)
    carry_pts += chunk_pts;
    if (in) {
      navgpu_sample_terms o;
      for (int k = 0; k < 5; ++k) {
        const bool seen = scored && t.scale[k] != 0 && k + 1 <= rec.first_fail;
        o.critic[k] = !seen ? __builtin_nan("") : (k + 1 == rec.first_fail ? (double)rec.fail_code : rec.v[k]);
      }
      o.cost_full = full;
      o.cost_ref = ref;
      o.first_fail = rec.first_fail;
      o.status = rec.status;
      o.n_points = rec.n_points;
      o.member = member ? 1 : 0;
      o.point_offset = off;
      o.reserved = 0;
      t.out[i] = o;
    }
  }
  if (tid == 0) {
    t.totals[0] = carry_pts;
    t.totals[1] = (uint32_t)max(n, 0);
  }
}
void launch_traj_scan(const PlannerDev& pl, const TrajCloudDev& t, uint32_t inst, hipStream_t s) {
  hipLaunchKernelGGL(k_traj_scan, dim3(1), dim3(kTrajScanThreads), 0, s, pl, t, inst);
}

// ------------------------------------------------------------------------------------------------
// k_traj_emit: a workgroup takes slots_per_group consecutive slots, a lane per slot.  The lane of a member slot rolls the
// trajectory - SimpleTrajectoryGenerator::generateTrajectory / computeNewPositions / computeNewVelocities
// (simple_trajectory_generator.cpp:218-276) step for step as scoreSamples and k_select roll it: fp64 on fp32 state,
// rollout_trig, continued acceleration - and writes its points to LDS at the slot's offset inside the workgroup's range of the
// cloud, which is contiguous; the workgroup then streams the range out, consecutive lanes to consecutive words.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTrajEmitThreads) void k_traj_emit(PlannerDev pl, TrajCloudDev t, uint32_t inst, uint32_t n_slots) {
  extern __shared__ __align__(16) float s_pts[];  // [slots_per_group * max_sim_steps][7]
  __shared__ uint32_t s_range[2];
  const uint32_t tid = threadIdx.x;
  const navgpu_dwa_config& c = pl.cfg;
  const uint32_t first_slot = blockIdx.x * t.slots_per_group;
  const uint32_t end_slot = min(first_slot + t.slots_per_group, n_slots);
  const uint32_t slot = first_slot + tid;
  const uint32_t lds_points = t.slots_per_group * pl.max_sim_steps;
  uint32_t my_off = 0;
  int my_n = 0;
  float cost = 0.f;
  if (tid < t.slots_per_group && slot < end_slot) {
    const navgpu_sample_terms o = t.out[slot];
    my_off = o.point_offset;
    my_n = o.member ? o.n_points : 0;
    cost = (float)(t.reference_costs ? o.cost_ref : o.cost_full);
    if (slot == first_slot) s_range[0] = my_off;
    if (slot == end_slot - 1) s_range[1] = my_off + (uint32_t)my_n;
  }
  __syncthreads();
  const uint32_t base = s_range[0], end = s_range[1];
  if (my_n > 0) {
    const navgpu_robot_state st = pl.state[inst];
    const int32_t* cnt = pl.axis_count + 4 * inst;
    const int nth = cnt[2], nyv = cnt[1];
    const int ix = (int)slot / (nyv * nth), rem = (int)slot - ix * (nyv * nth);
    const int iy = rem / nth, ith = rem - iy * nth;
    const float vs[3] = {pl.axis_samples[((size_t)inst * 3 + 0) * pl.max_axis + ix], pl.axis_samples[((size_t)inst * 3 + 1) * pl.max_axis + iy],
                         pl.axis_samples[((size_t)inst * 3 + 2) * pl.max_axis + ith]};
    const int num_steps = my_n;
    const double dt = c.sim_time / num_steps;
    const bool continued = !c.use_dwa;
    const RobotLimits& lim = pl.limits[inst];
    const float acc[3] = {(float)lim.acc_lim_x, (float)lim.acc_lim_y, (float)lim.acc_lim_theta};
    auto newVel = [&](const float* vel_in, float* out) {  // computeNewVelocities (:265-276)
      for (int i = 0; i < 3; ++i) {
        if (vel_in[i] < vs[i])
          out[i] = (float)fmin((double)vs[i], vel_in[i] + acc[i] * dt);
        else
          out[i] = (float)fmax((double)vs[i], vel_in[i] - acc[i] * dt);
      }
    };
    float lv[3] = {vs[0], vs[1], vs[2]};
    if (continued) {
      float t0[3];
      newVel(st.vel, t0);
      lv[0] = t0[0];
      lv[1] = t0[1];
      lv[2] = t0[2];
    }
    float px = st.pos[0], py = st.pos[1], pth = st.pos[2];
    const uint32_t local = my_off - base;
    for (int step = 0; step < num_steps; ++step) {
      if (local + (uint32_t)step < lds_points) {  // (always: a slot has at most max_sim_steps points)
        float* p = s_pts + (size_t)(local + step) * kTrajPointFloats;
        p[0] = px;
        p[1] = py;
        p[2] = 0.f;
        p[3] = pth;
        p[4] = 0.f;
        p[5] = 0.f;
        p[6] = cost;
      }
      if (continued) {
        float t1[3];
        newVel(lv, t1);
        lv[0] = t1[0];
        lv[1] = t1[1];
        lv[2] = t1[2];
      }
      // computeNewPositions (:253-260): fp64 on fp32 state, rounded back to fp32
      const double th = pth;
      double sn, cs, sn2 = 0.0, cs2 = 0.0;
      sincos(th, &sn, &cs);
      if (lv[1] != 0.0f) sincos(M_PI_2 + th, &sn2, &cs2);
      const double tx = c.rollout_trig ? (double)(lv[0] * (float)cs) : lv[0] * cs, ty = c.rollout_trig ? (double)(lv[0] * (float)sn) : lv[0] * sn;
      const float nxp = (float)(px + (tx + lv[1] * cs2) * dt);
      const float nyp = (float)(py + (ty + lv[1] * sn2) * dt);
      const float ntp = (float)(pth + lv[2] * dt);
      px = nxp;
      py = nyp;
      pth = ntp;
    }
  }
  __syncthreads();
  // the range [base, end) of the cloud, cut at the buffer's capacity
  const size_t g0 = (size_t)base * kTrajPointFloats;
  const size_t g_end = (size_t)min(end, t.capacity) * kTrajPointFloats;
  const uint32_t n_words = min(end - base, lds_points) * kTrajPointFloats;
  for (uint32_t i = tid; i < n_words; i += kTrajEmitThreads)
    if (g0 + i < g_end) t.points[g0 + i] = s_pts[i];
}
// slots of a k_traj_emit workgroup: as many as keep its points within 60 KB of LDS, at most a lane each
uint32_t traj_emit_slots_per_group(uint32_t max_sim_steps) {
  const size_t per_slot = (size_t)std::max(max_sim_steps, 1u) * kTrajPointFloats * sizeof(float);
  if (per_slot > 150u * 1024u) return 0;
  return (uint32_t)std::min<size_t>(kTrajEmitThreads, std::max<size_t>(1, (60u * 1024u) / per_slot));
}
void launch_traj_emit(const PlannerDev& pl, const TrajCloudDev& t, uint32_t inst, uint32_t n_slots, hipStream_t s) {
  if (!n_slots || !t.slots_per_group) return;
  const size_t lds = (size_t)t.slots_per_group * pl.max_sim_steps * kTrajPointFloats * sizeof(float);
  launchScore(k_traj_emit, dim3((n_slots + t.slots_per_group - 1) / t.slots_per_group), kTrajEmitThreads, lds, s, pl, t, inst, n_slots);
}

}  // namespace navgpu
