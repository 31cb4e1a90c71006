// HIP kernels (gfx950) for the legacy base_local_planner::TrajectoryPlanner:
//   k_tp_within  : MapCell::within_robot bits of path_map_ from the footprint cells the host rasterised
//                  (FootprintHelper::getFootprintCells with fill, trajectory_planner.cpp:918-930)
//   k_tp_rollout : TrajectoryPlanner::generateTrajectory (trajectory_planner.cpp:214-370), one lane per call of
//                  createTrajectories, fp64 state as in the reference; second pass stores the winner's points.  The rules
//                  of a step are those of tp_world_dev.h, shared with k_tp_probe (tp_probe_kernels.hip)
// The two MapGrid wavefronts are the k_bfs* kernels of planner_kernels.hip (bfs_grids = 2, `within` set).
// Compiled with -ffp-contract=off.
#include "tp_world_dev.h"

namespace navgpu {

__global__ void k_tp_within(PlannerDev pl, TpDev tp, uint32_t first) {
  const uint32_t inst = first + blockIdx.y;
  const uint32_t W = (pl.nx + 31) >> 5;
  const uint32_t n = tp.within_count[inst];
  uint32_t* bits = tp.within_bits + (size_t)inst * pl.ny * W;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t cell = tp.within_cells[(size_t)inst * tp.max_within + i];
    const uint32_t my = cell / pl.nx, mx = cell - my * pl.nx;
    atomicOr(&bits[my * W + (mx >> 5)], 1u << (mx & 31));
  }
}

void launch_tp_within(const PlannerDev& pl, const TpDev& tp, uint32_t first, uint32_t count, hipStream_t s) {
  const uint32_t W = (pl.nx + 31) / 32;
  hipMemsetAsync(tp.within_bits + (size_t)first * pl.ny * W, 0, sizeof(uint32_t) * (size_t)count * pl.ny * W, s);
  hipLaunchKernelGGL(k_tp_within, dim3(4, count), dim3(256), 0, s, pl, tp, first);
}

__global__ __launch_bounds__(128) void k_tp_rollout(PlannerDev pl, TpDev tp, uint32_t first, int store_points) {
  const uint32_t inst = first + blockIdx.y;
  const navgpu_tp_config& c = tp.cfg;
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (store_points) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    s = tp.winner[inst];
    if (s < 0) return;
  } else if (s >= (int)tp.n_samples[inst]) {
    return;
  }
  const TpRobot R = tpRobot(pl, tp, inst);
  const double* st = tp.start + (size_t)inst * 6;
  const double* smp = tp.samples + ((size_t)inst * tp.max_samples + s) * 3;
  const double vx_samp = smp[0], vy_samp = smp[1], vtheta_samp = smp[2];
  double* pts = tp.points + (size_t)inst * pl.max_sim_steps * 3;

  TpPose p{st[0], st[1], st[2], st[3], st[4], st[5], 0.0};
  const int num_steps = tpNumSteps(c, vx_samp, vy_samp, vtheta_samp);
  const double dt = c.sim_time / num_steps;
  double heading_diff = 0.0, path_dist = 0.0, goal_dist = 0.0, occ_cost = 0.0;
  double cost = -1.0;
  double ex = 0, ey = 0, eth = 0;
  int n_points = 0;
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
    ex = p.x;
    ey = p.y;
    eth = p.theta;
    if (store_points && n_points < (int)pl.max_sim_steps) {
      pts[3 * n_points] = p.x;
      pts[3 * n_points + 1] = p.y;
      pts[3 * n_points + 2] = p.theta;
    }
    ++n_points;
    tpAdvance(p, c, vx_samp, vy_samp, vtheta_samp, dt);
  }
  if (finished) cost = tpFinalCost(c, path_dist, goal_dist, occ_cost, heading_diff);
  if (store_points) return;
  TpOut o;
  o.cost = cost;
  o.ex = ex;
  o.ey = ey;
  o.eth = eth;
  o.n_points = n_points;
  o.ahead = 0.0;
  o.ahead_ok = 0;
  if (n_points > 0) {  // createTrajectories :680-688: goal_map_ at the heading_lookahead point of the endpoint
    const double x_r = ex + c.heading_lookahead * cos(eth), y_r = ey + c.heading_lookahead * sin(eth);
    uint32_t cell_x, cell_y;
    if (worldToMap(R.wm.g, x_r, y_r, cell_x, cell_y)) {
      o.ahead = (double)R.dgoal[cell_y * pl.nx + cell_x];
      o.ahead_ok = 1;
    }
  }
  tp.out[(size_t)inst * tp.max_samples + s] = o;
}

void launch_tp_rollout(const PlannerDev& pl, const TpDev& tp, uint32_t first, uint32_t count, int store_points, hipStream_t s) {
  const uint32_t blocks = store_points ? 1u : (tp.max_samples + 127u) / 128u;
  hipLaunchKernelGGL(k_tp_rollout, dim3(blocks, count), dim3(128), 0, s, pl, tp, first, store_points);
}

}  // namespace navgpu
