// What the kernels of the legacy base_local_planner::TrajectoryPlanner share (tp_kernels.hip: k_tp_rollout, one lane per
// generateTrajectory call; tp_probe_kernels.hip: k_tp_probe, one wave per call and one lane per step): the planner's view of the
// world, and generateTrajectory (trajectory_planner.cpp:214-370) cut into its three rules - what one step decides (tpEvalStep), how
// the pose moves on to the next step (tpAdvance) and the cost of a trajectory that ran to its end (tpFinalCost).  One copy of each.
// Compiled with -ffp-contract=off.
#pragma once
#include "costmap_model_dev.h"

namespace navgpu {

// CostmapModel on the global costmap (costmap_model_dev.h) + the planner's own ray walk for heading scoring
struct TpWorld : CostmapModelDev {
  // TrajectoryPlanner::pointCost / lineCost (trajectory_planner.cpp:388-472): the planner's own ray walk for headingDiff;
  // unlike CostmapModel::pointCost it fails on INSCRIBED cells too
  __device__ double planLineCost(int x0, int x1, int y0, int y1) const {
    return lineMax(x0, y0, x1, y1, [&](uint8_t cost) { return cost == kLethal || cost == kInscribed || (cost == kNoInfo && !allow_unknown); });
  }
  // TrajectoryPlanner::headingDiff (:372-386): the farthest plan pose with a clear line of sight from the robot's cell
  __device__ double headingDiff(int cell_x, int cell_y, double x, double y, double heading, const double* plan, uint32_t n_plan) const {
    for (int i = (int)n_plan - 1; i >= 0; --i) {
      uint32_t gx_c, gy_c;
      if (worldToMap(g, plan[2 * i], plan[2 * i + 1], gx_c, gy_c)) {
        if (planLineCost(cell_x, (int)gx_c, cell_y, (int)gy_c) >= 0) {
          const double gx = g.ox + (gx_c + 0.5) * g.res, gy = g.oy + (gy_c + 0.5) * g.res;  // mapToWorld
          // angles::shortest_angular_distance(heading, atan2(..)) = normalize_angle(to - from), fmod form
          const double a = atan2(gy - y, gx - x) - heading;
          double r = fmod(fmod(a, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI);
          if (r > M_PI) r -= 2.0 * M_PI;
          return fabs(r);
        }
      }
    }
    return 1.7976931348623157e308;  // DBL_MAX
  }
};

__device__ __forceinline__ double tpNewVelocity(double vg, double vi, double a_max, double dt) {  // trajectory_planner.h:369-374
  if ((vg - vi) >= 0) return fmin(vg, vi + a_max * dt);
  return fmax(vg, vi - a_max * dt);
}

// one robot as generateTrajectory sees it: costmap, the two MapGrids, footprint and plan
struct TpRobot {
  TpWorld wm;
  const uint32_t *dpath, *dgoal;  // path_map_ / goal_map_ target distances
  const double* spec;             // footprint_spec
  uint32_t nfp;
  const double* plan;             // global_plan_ as x, y pairs
  uint32_t n_plan;
  double impossible_cost;         // path_map_.obstacleCosts()
};
__device__ __forceinline__ TpRobot tpRobot(const PlannerDev& pl, const TpDev& tp, uint32_t inst) {
  TpRobot r;
  r.wm.master = pl.master + (size_t)inst * pl.cells_padded;
  r.wm.g = Geom{pl.origin[2 * inst], pl.origin[2 * inst + 1], pl.res, pl.nx, pl.ny};
  r.wm.allow_unknown = tp.cfg.allow_unknown != 0;
  r.dpath = pl.path + (size_t)inst * pl.cells;
  r.dgoal = pl.goal + (size_t)inst * pl.cells;
  r.spec = pl.fp_spec + (size_t)inst * kMaxFootprint * 2;
  r.nfp = pl.fp_n[inst];
  r.plan = pl.plan + (size_t)inst * pl.max_plan * 2;
  r.n_plan = pl.plan_count[inst];
  r.impossible_cost = (double)pl.cells;
  return r;
}

// the simulated state at one step (:225-233, :252, and the loop's own updates)
struct TpPose {
  double x, y, theta, vx, vy, vtheta, time;
};
// num_steps of a sample (:236-249)
__device__ __forceinline__ int tpNumSteps(const navgpu_tp_config& c, double vx_samp, double vy_samp, double vtheta_samp) {
  const double vmag = hypot(vx_samp, vy_samp);
  int num_steps;
  if (!c.heading_scoring)
    num_steps = int(fmax((vmag * c.sim_time) / c.sim_granularity, fabs(vtheta_samp) / c.angular_sim_granularity) + 0.5);
  else
    num_steps = int(c.sim_time / c.sim_granularity + 0.5);
  if (num_steps == 0) num_steps = 1;
  return num_steps;
}
// The end of a step (:348-359): new velocities under the acceleration limits, then the new pose.  Nothing here reads the costmap:
// the pose sequence follows from the start state, the sample and dt alone.
__device__ __forceinline__ void tpAdvance(TpPose& p, const navgpu_tp_config& c, double vx_samp, double vy_samp, double vtheta_samp, double dt) {
  p.vx = tpNewVelocity(vx_samp, p.vx, c.acc_lim_x, dt);
  p.vy = tpNewVelocity(vy_samp, p.vy, c.acc_lim_y, dt);
  p.vtheta = tpNewVelocity(vtheta_samp, p.vtheta, c.acc_lim_theta, dt);
  const double nx_ = p.x + (p.vx * cos(p.theta) + p.vy * cos(M_PI_2 + p.theta)) * dt;  // computeNewXPosition
  const double ny_ = p.y + (p.vx * sin(p.theta) + p.vy * sin(M_PI_2 + p.theta)) * dt;
  p.theta = p.theta + p.vtheta * dt;
  p.x = nx_;
  p.y = ny_;
  p.time += dt;
}

// what one step that did not fail hands to the trajectory: the larger of footprint cost and centre cell (occ_cost is the maximum
// of these over the steps, :307) and the distances it set, if any
struct TpStep {
  double occ, path_dist, goal_dist, heading_diff;
  bool set_path, set_goal, set_heading;
};
// The body of one step (:268-342).  Returns 0, or what cost_ becomes when the trajectory ends here: -1 (the pose is off the map, or the
// footprint is in collision), -2 (no path from this cell to the plan or the goal).
__device__ __forceinline__ int tpEvalStep(const TpRobot& r, const navgpu_tp_config& c, const TpPose& p, double dt, TpStep& o) {
  o.set_path = o.set_goal = o.set_heading = false;
  o.occ = o.path_dist = o.goal_dist = o.heading_diff = 0.0;
  uint32_t cell_x, cell_y;
  if (!worldToMap(r.wm.g, p.x, p.y, cell_x, cell_y)) return -1;
  const double footprint_cost = r.wm.footprintCost(p.x, p.y, p.theta, r.spec, r.nfp);
  if (footprint_cost < 0) return -1;
  o.occ = fmax(footprint_cost, double(r.wm.master[cell_y * r.wm.g.nx + cell_x]));
  if (c.simple_attractor) {  // :310-315 (the host refuses an empty plan)
    const double gx = r.plan[2 * (r.n_plan - 1)], gy = r.plan[2 * (r.n_plan - 1) + 1];
    o.goal_dist = (p.x - gx) * (p.x - gx) + (p.y - gy) * (p.y - gy);
    o.set_goal = true;
    return 0;
  }
  if (c.heading_scoring) {  // :321-327: the distances are taken at the one step whose time falls in the window
    if (!(p.time >= c.heading_scoring_timestep && p.time < c.heading_scoring_timestep + dt)) return 0;
    o.heading_diff = r.wm.headingDiff((int)cell_x, (int)cell_y, p.x, p.y, p.theta, r.plan, r.n_plan);
    o.set_heading = true;
  }
  o.path_dist = (double)r.dpath[cell_y * r.wm.g.nx + cell_x];
  o.goal_dist = (double)r.dgoal[cell_y * r.wm.g.nx + cell_x];
  o.set_path = o.set_goal = true;
  if (r.impossible_cost <= o.goal_dist || r.impossible_cost <= o.path_dist) return -2;
  return 0;
}
// cost_ of a trajectory whose every step passed (:363-369)
__device__ __forceinline__ double tpFinalCost(const navgpu_tp_config& c, double path_dist, double goal_dist, double occ_cost, double heading_diff) {
  return !c.heading_scoring ? c.pdist_scale * path_dist + goal_dist * c.gdist_scale + c.occdist_scale * occ_cost
                            : c.occdist_scale * occ_cost + c.pdist_scale * path_dist + 0.3 * heading_diff + goal_dist * c.gdist_scale;
}

}  // namespace navgpu
