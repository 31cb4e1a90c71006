// HIP kernel (gfx950) behind navgpu_tp_score_trajectories: TrajectoryPlanner::scoreTrajectory (trajectory_planner.cpp:502-531, which is
// generateTrajectory, :214-370, for one sample) for a list of probes.
//   k_tp_probe : one wave64 workgroup per probe, one lane per step of its trajectory.
// generateTrajectory's loop looks serial, but its pose sequence does not depend on the costmap: x_i, y_i, theta_i, v*_i and `time` follow
// from the start state, the sample and dt; only the early exit reads the map.  So EVERY LANE ITERATES THE POSE RECURRENCE TO ITS OWN
// STEP (tpAdvance, the operations and the order of k_tp_rollout: lane l has taken l advances when chunk 0 is evaluated and takes 64 more
// per chunk; no LDS, no barrier), and lane l evaluates step 64 * chunk + l with tpEvalStep.  A trajectory fails at its FIRST failing
// step: the lowest set bit of the 64-bit ballot over the chunk, whose code is the answer; later chunks are not evaluated.  Without a
// failure occ_cost is a maximum (exact in any order: the values are cell bytes), path_dist / goal_dist / heading_diff are those of the
// highest-numbered step that set them, and the cost is tpFinalCost of them.  Nothing is accumulated in floating point across steps, so the
// answer is bit-equal to the one lane of k_tp_rollout that navgpu_tp_score_trajectory runs.
// Compiled with -ffp-contract=off.
#include "tp_world_dev.h"

namespace navgpu {

__global__ __launch_bounds__(64) void k_tp_probe(PlannerDev pl, TpDev tp, TpProbeBatch pb) {
  const uint32_t q = blockIdx.x;
  if (q >= pb.n_probes) return;
  const int lane = (int)threadIdx.x;
  const navgpu_tp_config& c = tp.cfg;
  const TpRobot R = tpRobot(pl, tp, pb.instance[q]);
  const double* in = pb.probes + (size_t)q * 9;  // pose x y theta, velocity x y theta, sample x y theta
  const double vx_samp = in[6], vy_samp = in[7], vtheta_samp = in[8];
  TpPose p{in[0], in[1], in[2], in[3], in[4], in[5], 0.0};
  const int num_steps = tpNumSteps(c, vx_samp, vy_samp, vtheta_samp);
  const double dt = c.sim_time / num_steps;
  for (int k = 0; k < lane && k < num_steps; ++k) tpAdvance(p, c, vx_samp, vy_samp, vtheta_samp, dt);

  double occ_cost = 0.0, path_dist = 0.0, goal_dist = 0.0, heading_diff = 0.0;  // occ_cost: this lane's steps; the others: wave-uniform
  double cost = 0.0;
  bool finished = true;
  for (int base = 0; base < num_steps; base += 64) {
    const bool live = base + lane < num_steps;
    TpStep step;
    step.occ = step.path_dist = step.goal_dist = step.heading_diff = 0.0;
    step.set_path = step.set_goal = step.set_heading = false;
    const int code = live ? tpEvalStep(R, c, p, dt, step) : 0;
    const unsigned long long failed = __ballot(code != 0);
    if (failed) {  // the first failing step ends the trajectory with its code
      cost = (double)__shfl(code, __ffsll((long long)failed) - 1);
      finished = false;
      break;
    }
    occ_cost = fmax(occ_cost, step.occ);
    // the chunks rise, so the highest lane of the latest chunk that set a value is the highest-numbered such step
    const unsigned long long m_path = __ballot(step.set_path), m_goal = __ballot(step.set_goal), m_head = __ballot(step.set_heading);
    if (m_path) path_dist = __shfl(step.path_dist, 63 - __clzll((long long)m_path));
    if (m_goal) goal_dist = __shfl(step.goal_dist, 63 - __clzll((long long)m_goal));
    if (m_head) heading_diff = __shfl(step.heading_diff, 63 - __clzll((long long)m_head));
    if (base + 64 < num_steps)
      for (int k = 0; k < 64 && base + lane + k < num_steps; ++k) tpAdvance(p, c, vx_samp, vy_samp, vtheta_samp, dt);
  }
  if (finished) {
    for (int d = 32; d > 0; d >>= 1) occ_cost = fmax(occ_cost, __shfl_xor(occ_cost, d));
    cost = tpFinalCost(c, path_dist, goal_dist, occ_cost, heading_diff);
  }
  if (lane == 0) pb.cost[q] = cost;
}

void launch_tp_probe(const PlannerDev& pl, const TpDev& tp, const TpProbeBatch& pb, hipStream_t s) {
  hipLaunchKernelGGL(k_tp_probe, dim3(pb.n_probes), dim3(64), 0, s, pl, tp, pb);
}

}  // namespace navgpu
