// EXPERIMENT, not part of libnavgpu.so: the other work split of navgpu_tp_score_trajectories' kernel, one LANE per probe - the serial
// loop of k_tp_rollout (tp_kernels.hip) pointed at the probe buffers - in place of k_tp_probe's wave per probe and lane per step
// (navigation_amd/csrc/tp_probe_kernels.hip).  Same rules (tp_world_dev.h), same answers; 256 probes are 4 waves here and 256 there.
//   make -C navigation_amd/csrc tp-probe-ab   links it into navigation_amd/libnavgpu_lpp.so in place of tp_probe_kernels.o
//   tools/bench_tp_ros.py --ab                times both libraries
// Compiled with -ffp-contract=off.
#include "tp_world_dev.h"

namespace navgpu {

__global__ __launch_bounds__(128) void k_tp_probe_lanes(PlannerDev pl, TpDev tp, TpProbeBatch pb) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= pb.n_probes) return;
  const navgpu_tp_config& c = tp.cfg;
  const TpRobot R = tpRobot(pl, tp, pb.instance[q]);
  const double* in = pb.probes + (size_t)q * 9;
  const double vx_samp = in[6], vy_samp = in[7], vtheta_samp = in[8];
  TpPose p{in[0], in[1], in[2], in[3], in[4], in[5], 0.0};
  const int num_steps = tpNumSteps(c, vx_samp, vy_samp, vtheta_samp);
  const double dt = c.sim_time / num_steps;
  double heading_diff = 0.0, path_dist = 0.0, goal_dist = 0.0, occ_cost = 0.0, cost = 0.0;
  bool finished = true;
  for (int i = 0; i < num_steps; ++i) {
    TpStep step;
    const int code = tpEvalStep(R, c, p, dt, step);
    if (code) {
      cost = (double)code;
      finished = false;
      break;
    }
    occ_cost = fmax(occ_cost, step.occ);
    if (step.set_heading) heading_diff = step.heading_diff;
    if (step.set_path) path_dist = step.path_dist;
    if (step.set_goal) goal_dist = step.goal_dist;
    tpAdvance(p, c, vx_samp, vy_samp, vtheta_samp, dt);
  }
  if (finished) cost = tpFinalCost(c, path_dist, goal_dist, occ_cost, heading_diff);
  pb.cost[q] = cost;
}

void launch_tp_probe(const PlannerDev& pl, const TpDev& tp, const TpProbeBatch& pb, hipStream_t s) {
  hipLaunchKernelGGL(k_tp_probe_lanes, dim3((pb.n_probes + 127u) / 128u), dim3(128), 0, s, pl, tp, pb);
}

}  // namespace navgpu
