// Working stand-in for the generated <base_local_planner/BaseLocalPlannerConfig.h>, for tools/tp_reference_harness.cpp only: the fields
// of cfg/BaseLocalPlanner.cfg with the types that file gives them (heading_scoring_timestep is a double).  Goes before tests/ros_stubs
// on the include path.
#pragma once
#include <string>
namespace base_local_planner {
struct BaseLocalPlannerConfig {
  double acc_lim_x, acc_lim_y, acc_lim_theta, max_vel_x, min_vel_x, max_vel_theta, min_vel_theta, min_in_place_vel_theta, sim_time,
      sim_granularity, angular_sim_granularity, pdist_scale, gdist_scale, occdist_scale, oscillation_reset_dist, escape_reset_dist,
      escape_reset_theta, heading_lookahead, escape_vel, heading_scoring_timestep;
  int vx_samples, vtheta_samples;
  bool holonomic_robot, heading_scoring, simple_attractor, dwa, restore_defaults;
  std::string y_vels;
  BaseLocalPlannerConfig() {}
};
}  // namespace base_local_planner
