// HIP kernels (gfx950) for the legacy base_local_planner::TrajectoryPlanner:
//   k_tp_within  : MapCell::within_robot bits of path_map_ from the footprint cells the host rasterised
//                  (FootprintHelper::getFootprintCells with fill, trajectory_planner.cpp:918-930)
//   k_tp_stage_scatter, k_tp_gather_out, k_tp_winner_scatter : what a listed call hands over and reads back, one block each way
//   k_tp_rollout : TrajectoryPlanner::generateTrajectory (trajectory_planner.cpp:214-370), one lane per call of
//                  createTrajectories, fp64 state as in the reference; second pass stores the winner's points.  The rules
//                  of a step are those of tp_world_dev.h, shared with k_tp_probe (tp_probe_kernels.hip)
// The two MapGrid wavefronts are the k_bfs* kernels of planner_kernels.hip (bfs_grids = 2, `within` set).
// Compiled with -ffp-contract=off.
#include "tp_world_dev.h"

namespace navgpu {

// Which robot a block row of these kernels belongs to: RobotRange (navgpu_tp_find_best_path) or RobotList (its listed form), one
// copy of each body (navgpu_device.h).
template <class Robots>
__global__ void k_tp_within(PlannerDev pl, TpDev tp, Robots robots) {
  const uint32_t inst = robots(blockIdx.y);
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
  hipLaunchKernelGGL(k_tp_within<RobotRange>, dim3(4, count), dim3(256), 0, s, pl, tp, RobotRange{first});
}
// the listed form: k_tp_stage_scatter in front of it has cleared the listed robots' bitmaps
void launch_tp_within_list(const PlannerDev& pl, const TpDev& tp, const uint32_t* list, uint32_t count, hipStream_t s) {
  hipLaunchKernelGGL(k_tp_within<RobotList>, dim3(4, count), dim3(256), 0, s, pl, tp, RobotList{list});
}

template <class Robots>
__global__ __launch_bounds__(128) void k_tp_rollout(PlannerDev pl, TpDev tp, Robots robots, int store_points) {
  const uint32_t inst = robots(blockIdx.y);
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
  hipLaunchKernelGGL(k_tp_rollout<RobotRange>, dim3(blocks, count), dim3(128), 0, s, pl, tp, RobotRange{first}, store_points);
}
void launch_tp_rollout_list(const PlannerDev& pl, const TpDev& tp, const uint32_t* list, uint32_t count, int store_points, hipStream_t s) {
  const uint32_t blocks = store_points ? 1u : (tp.max_samples + 127u) / 128u;
  hipLaunchKernelGGL(k_tp_rollout<RobotList>, dim3(blocks, count), dim3(128), 0, s, pl, tp, RobotList{list}, store_points);
}

// k_tp_stage_scatter: the packed upload of a listed call (TpStageBlock) into the slots of its robots - block row k serves record k.
// Plan points and their count always; with_rollout also the samples, the cells under the robot, their counts and the start state,
// and the robot's within_robot bitmap is cleared for the k_tp_within behind this launch.  A value has one writer: plain stores.
// The counts are the host's, checked against the capacities before the upload; they are clamped here all the same.
constexpr uint32_t kTpStageBlocks = 8, kTpStageThreads = 256;
__global__ __launch_bounds__(kTpStageThreads) void k_tp_stage_scatter(PlannerDev pl, TpDev tp, TpStageBlock b, int with_rollout) {
  const TpStageRec r = b.rec[blockIdx.y];
  const uint32_t inst = r.inst;
  const uint32_t t0 = blockIdx.x * kTpStageThreads + threadIdx.x, stride = kTpStageBlocks * kTpStageThreads;
  const uint32_t n_plan = min(r.n_plan, pl.max_plan);
  double* plan = pl.plan + (size_t)inst * pl.max_plan * 2;
  const double* plan_in = b.plan + (size_t)r.plan_off * 2;
  for (uint32_t i = t0; i < 2 * n_plan; i += stride) plan[i] = plan_in[i];
  if (t0 == 0) pl.plan_count[inst] = n_plan;
  if (!with_rollout) return;
  const uint32_t n_samples = min(r.n_samples, tp.max_samples), n_within = min(r.n_within, tp.max_within);
  double* smp = tp.samples + (size_t)inst * tp.max_samples * 3;
  const double* smp_in = b.samples + (size_t)r.samples_off * 3;
  for (uint32_t i = t0; i < 3 * n_samples; i += stride) smp[i] = smp_in[i];
  uint32_t* cells = tp.within_cells + (size_t)inst * tp.max_within;
  const uint32_t* cells_in = b.within + r.within_off;
  for (uint32_t i = t0; i < n_within; i += stride) cells[i] = cells_in[i];
  const uint32_t words = pl.ny * ((pl.nx + 31) >> 5);
  uint32_t* bits = tp.within_bits + (size_t)inst * words;
  for (uint32_t i = t0; i < words; i += stride) bits[i] = 0u;
  if (t0 < 6) tp.start[(size_t)inst * 6 + t0] = b.rec[blockIdx.y].start[t0];
  if (t0 == 6) tp.n_samples[inst] = n_samples;
  if (t0 == 7) tp.within_count[inst] = n_within;
}
void launch_tp_stage_scatter(const PlannerDev& pl, const TpDev& tp, const TpStageBlock& b, uint32_t n_robots, int with_rollout, hipStream_t s) {
  hipLaunchKernelGGL(k_tp_stage_scatter, dim3(kTpStageBlocks, n_robots), dim3(kTpStageThreads), 0, s, pl, tp, b, with_rollout);
}

// k_tp_gather_out: the first pass's results of the listed robots, packed in the order of the upload's samples, for one read-back
__global__ __launch_bounds__(128) void k_tp_gather_out(TpDev tp, const TpStageRec* rec, TpOut* packed) {
  const TpStageRec& r = rec[blockIdx.y];
  const uint32_t s = blockIdx.x * 128 + threadIdx.x;
  if (s >= min(r.n_samples, tp.max_samples)) return;
  packed[r.samples_off + s] = tp.out[(size_t)r.inst * tp.max_samples + s];
}
void launch_tp_gather_out(const TpDev& tp, const TpStageRec* rec, TpOut* packed, uint32_t n_robots, hipStream_t s) {
  hipLaunchKernelGGL(k_tp_gather_out, dim3((tp.max_samples + 127u) / 128u, n_robots), dim3(128), 0, s, tp, rec, packed);
}
// k_tp_winner_scatter: the second pass's winners, uploaded by list position, into the robots' slots
__global__ __launch_bounds__(256) void k_tp_winner_scatter(TpDev tp, const uint32_t* list, const int32_t* winners, uint32_t n_robots) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k < n_robots) tp.winner[list[k]] = winners[k];
}
void launch_tp_winner_scatter(const TpDev& tp, const uint32_t* list, const int32_t* winners, uint32_t n_robots, hipStream_t s) {
  hipLaunchKernelGGL(k_tp_winner_scatter, dim3((n_robots + 255u) / 256u), dim3(256), 0, s, tp, list, winners, n_robots);
}

}  // namespace navgpu
