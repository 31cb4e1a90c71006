// Host-side mirror of TrajectoryPlannerROS's control cycle for a fleet (include/navgpu.h, navgpu_tp_ros_*;
// base_local_planner/src/trajectory_planner_ros.cpp:283-597): plan window, goal test on the window's last pose, the stop / rotate
// candidates and the dispatch to the navgpu_tp_* core - plain host arithmetic in fp64; the grids, the rollout and the candidates' legality
// run on the GPU through navgpu_tp_update_plans, navgpu_tp_find_best_path and navgpu_tp_score_trajectories.
// updatePlan + findBestPath run ONCE per call for the robots that need them: through the range calls when those robots form one
// contiguous run, else through navgpu_tp_update_plans_list / navgpu_tp_find_best_path_list - a robot that is at its goal, or has no
// window, costs no launch.
#include "navgpu_fleet.h"

extern "C" {

static double tprSign(double x) { return x < 0.0 ? -1.0 : 1.0; }  // base_local_planner sign() (trajectory_planner_ros.h:192-194)
static bool tprStopped(const double v[3], double rot_stopped, double trans_stopped) {  // goal_functions.cpp:249-254
  return fabs(v[2]) <= rot_stopped && fabs(v[0]) <= trans_stopped && fabs(v[1]) <= trans_stopped;
}

int navgpu_tp_ros_candidate(const navgpu_tp_config* c, int32_t rotate, const double pose[3], const double odom_vel[3], double goal_th,
                            double vs[3]) {
  if (!c || !pose || !odom_vel || !vs) return NAVGPU_ERR_INVALID;
  const double vel_yaw = odom_vel[2];
  if (!rotate) {  // stopWithAccLimits (:283-290)
    vs[0] = tprSign(odom_vel[0]) * std::max(0.0, (fabs(odom_vel[0]) - c->acc_lim_x * c->sim_period));
    vs[1] = tprSign(odom_vel[1]) * std::max(0.0, (fabs(odom_vel[1]) - c->acc_lim_y * c->sim_period));
    vs[2] = tprSign(vel_yaw) * std::max(0.0, (fabs(vel_yaw) - c->acc_lim_theta * c->sim_period));
    return NAVGPU_OK;
  }
  // rotateToGoal (:312-337)
  const double yaw = pose[2];
  const double ang_diff = navgpu_shortest_angular_distance(yaw, goal_th);
  double v_theta_samp = ang_diff > 0.0 ? std::min(c->max_vel_th, std::max(c->min_in_place_vel_th, ang_diff))
                                       : std::max(c->min_vel_th, std::min(-1.0 * c->min_in_place_vel_th, ang_diff));
  const double max_acc_vel = fabs(vel_yaw) + c->acc_lim_theta * c->sim_period;
  const double min_acc_vel = fabs(vel_yaw) - c->acc_lim_theta * c->sim_period;
  v_theta_samp = tprSign(v_theta_samp) * std::min(std::max(fabs(v_theta_samp), min_acc_vel), max_acc_vel);
  const double max_speed_to_stop = sqrt(2 * c->acc_lim_theta * fabs(ang_diff));
  v_theta_samp = tprSign(v_theta_samp) * std::min(max_speed_to_stop, fabs(v_theta_samp));
  // "Re-enforce min_in_place_vel_th_.  It is more important than the acceleration limits."
  v_theta_samp = v_theta_samp > 0.0 ? std::min(c->max_vel_th, std::max(c->min_in_place_vel_th, v_theta_samp))
                                    : std::max(c->min_vel_th, std::min(-1.0 * c->min_in_place_vel_th, v_theta_samp));
  vs[0] = 0.0;
  vs[1] = 0.0;
  vs[2] = v_theta_samp;
  return NAVGPU_OK;
}

int navgpu_tp_ros_configure(navgpu_fleet* f, const navgpu_tp_ros_params* p) {
  if (!f || !p) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tp_configured) return NAVGPU_ERR_STATE;
  f->tpr_params = *p;
  f->tpr_configured = true;
  if (f->tpr.size() != f->desc.n_instances) f->tpr.assign(f->desc.n_instances, navgpu_fleet::TpRosState());
  return NAVGPU_OK;
}

int navgpu_tp_ros_set_plans(navgpu_fleet* f, uint32_t first, uint32_t count, const double* poses, const uint32_t* offsets, const double* T) {
  if (!f || !offsets || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k)
    if (offsets[k + 1] < offsets[k]) return NAVGPU_ERR_INVALID;
  if (offsets[count] > offsets[0] && !poses) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tpr_configured) return NAVGPU_ERR_STATE;
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_fleet::TpRosState& st = f->tpr[first + k];
    const uint32_t n = offsets[k + 1] - offsets[k];
    const double* p = n ? poses + 3 * (size_t)offsets[k] : nullptr;
    st.plan.assign(p, p + 3 * (size_t)n);  // global_plan_ = orig_global_plan
    st.have_plan = true;
    st.has_T = T != nullptr;
    if (T) memcpy(st.T, T + 3 * (size_t)k, sizeof(st.T));
    st.xy_tolerance_latch = false;  // :366
    st.reached_goal = false;        // :368
  }
  return NAVGPU_OK;
}

static int tprCopyPlan(const std::vector<double>& pl, double* xyyaw, uint32_t capacity) {
  const uint32_t n = (uint32_t)(pl.size() / 3);
  if (xyyaw) {
    if (capacity < n) return NAVGPU_ERR_CAPACITY;
    if (n) memcpy(xyyaw, pl.data(), sizeof(double) * pl.size());
  }
  return (int)n;
}
int navgpu_tp_ros_get_plan(navgpu_fleet* f, uint32_t instance, double* xyyaw, uint32_t capacity) {
  if (!f || instance >= f->desc.n_instances) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tpr_configured) return NAVGPU_ERR_STATE;
  return tprCopyPlan(f->tpr[instance].plan, xyyaw, capacity);
}
int navgpu_tp_ros_transformed_plan(navgpu_fleet* f, uint32_t instance, double* xyyaw, uint32_t capacity) {
  if (!f || instance >= f->desc.n_instances) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tpr_configured) return NAVGPU_ERR_STATE;
  return tprCopyPlan(f->tpr[instance].transformed, xyyaw, capacity);
}

int navgpu_tp_ros_is_goal_reached(navgpu_fleet* f, uint32_t first, uint32_t count, int32_t* reached) {
  if (!f || !reached || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tpr_configured) return NAVGPU_ERR_STATE;
  for (uint32_t k = 0; k < count; ++k) reached[k] = f->tpr[first + k].reached_goal ? 1 : 0;  // :596
  return NAVGPU_OK;
}

int navgpu_tp_ros_compute_velocity_commands(navgpu_fleet* f, uint32_t first, uint32_t count, const navgpu_robot_input* in, navgpu_cmd_result* out) {
  if (!f || !in || !out || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tpr_configured || !f->tp_configured) return NAVGPU_ERR_STATE;
  const navgpu_tp_ros_params& prm = f->tpr_params;
  const navgpu_tp_config& cfg = f->tp.cfg;
  const uint32_t max_plan = f->pl.max_plan;
  const double dist_threshold = std::max(f->cm.nx * f->cm.res / 2.0, f->cm.ny * f->cm.res / 2.0);  // goal_functions.cpp:118-119
  enum { NONE = 0, ROLLOUT, REACHED, AT_GOAL };
  std::vector<uint8_t> kind(count, NONE);
  std::vector<double> window((size_t)max_plan * 3), goal_th(count, 0.0);
  // --- the window, the goal test and the at-goal answer per robot (:378-440)
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_fleet::TpRosState& st = f->tpr[first + k];
    navgpu_cmd_result& o = out[k];
    o = navgpu_cmd_result();
    st.transformed.clear();
    if (!in[k].have_pose) continue;                    // getRobotPose failed (:380-382)
    if (!st.have_plan || st.plan.empty()) continue;    // transformGlobalPlan: "Received plan with zero length" (:386-389)
    uint32_t n_loc = 0, n_er = 0;
    const int rc = navgpu_local_plan_window(st.plan.data(), (uint32_t)(st.plan.size() / 3), in[k].pose, st.has_T ? st.T : nullptr, dist_threshold,
                                            prm.prune_plan, window.data(), max_plan, &n_loc, &n_er);
    if (rc == NAVGPU_ERR_CAPACITY) return rc;
    if (rc != NAVGPU_OK) continue;
    if (n_er) st.plan.erase(st.plan.begin(), st.plan.begin() + 3 * (size_t)std::min<size_t>(n_er, st.plan.size() / 3));  // prunePlan (:392-393)
    st.transformed.assign(window.begin(), window.begin() + 3 * (size_t)n_loc);
    o.local_plan_points = (int32_t)n_loc;
    if (n_loc == 0) continue;                          // :408-409
    const double* goal = &st.transformed[3 * (size_t)(n_loc - 1)];  // transformed_plan.back() (:411-419)
    goal_th[k] = goal[2];
    kind[k] = ROLLOUT;
    if (st.xy_tolerance_latch || hypot(goal[0] - in[k].pose[0], goal[1] - in[k].pose[1]) <= prm.xy_goal_tolerance) {  // :422
      if (prm.latch_xy_goal_tolerance) st.xy_tolerance_latch = true;
      const double angle = navgpu_shortest_angular_distance(in[k].pose[2], goal_th[k]);
      if (fabs(angle) <= prm.yaw_goal_tolerance) {  // :432-439
        st.rotating_to_goal = false;
        st.xy_tolerance_latch = false;
        st.reached_goal = true;
        o.ok = 1;
        o.branch = NAVGPU_BRANCH_AT_GOAL;
        kind[k] = AT_GOAL;
      } else {
        kind[k] = REACHED;
      }
    }
  }
  // --- updatePlan(transformed_plan) + findBestPath (:443-444, :475-478) for every robot that is not at its goal: one of each
  std::vector<navgpu_tp_result> res(count);
  {
    std::vector<uint32_t> ks, inst, offsets(1, 0u);  // the robots by position in the call / in the fleet
    std::vector<navgpu_robot_state> states;
    std::vector<double> packed;
    for (uint32_t k = 0; k < count; ++k) {
      if (kind[k] != ROLLOUT && kind[k] != REACHED) continue;
      const std::vector<double>& t = f->tpr[first + k].transformed;
      for (size_t q = 0; q < t.size() / 3; ++q) {
        packed.push_back(t[3 * q]);
        packed.push_back(t[3 * q + 1]);
      }
      offsets.push_back((uint32_t)(packed.size() / 2));
      navgpu_robot_state s{};
      for (int a = 0; a < 3; ++a) {  // Eigen::Vector3f pos / vel (trajectory_planner.cpp:911-912)
        s.pos[a] = (float)in[k].pose[a];
        s.vel[a] = (float)in[k].odom_vel[a];
      }
      states.push_back(s);
      ks.push_back(k);
      inst.push_back(first + k);
    }
    if (!ks.empty()) {
      const uint32_t n = (uint32_t)ks.size();
      std::vector<navgpu_tp_result> got(n);
      int rc;
      if (ks.back() - ks.front() + 1 == n) {  // one contiguous run: the range calls
        rc = navgpu_tp_update_plans(f, inst[0], n, packed.data(), offsets.data(), 0);
        if (rc == NAVGPU_OK) rc = navgpu_tp_find_best_path(f, inst[0], n, states.data(), got.data());
      } else {
        rc = navgpu_tp_update_plans_list(f, n, inst.data(), packed.data(), offsets.data(), 0);
        if (rc == NAVGPU_OK) rc = navgpu_tp_find_best_path_list(f, n, inst.data(), states.data(), got.data());
      }
      if (rc != NAVGPU_OK) return rc;
      for (uint32_t q = 0; q < n; ++q) res[ks[q]] = got[q];
    }
  }
  // --- position reached (:447-464): the stop / rotate candidates, checked in ONE call against the grids findBestPath just made
  std::vector<uint32_t> chk_inst, chk_k, chk_off(1, 0u);
  std::vector<double> chk_probe;
  for (uint32_t k = 0; k < count; ++k) {
    if (kind[k] != REACHED) continue;
    navgpu_fleet::TpRosState& st = f->tpr[first + k];
    double vs[3];
    if (!st.rotating_to_goal && !tprStopped(in[k].odom_vel, prm.rot_stopped_velocity, prm.trans_stopped_velocity)) {
      navgpu_tp_ros_candidate(&cfg, 0, in[k].pose, in[k].odom_vel, goal_th[k], vs);
      out[k].branch = NAVGPU_BRANCH_STOP;
    } else {
      st.rotating_to_goal = true;  // :460
      navgpu_tp_ros_candidate(&cfg, 1, in[k].pose, in[k].odom_vel, goal_th[k], vs);
      out[k].branch = NAVGPU_BRANCH_ROTATE;
    }
    chk_inst.push_back(first + k);
    chk_k.push_back(k);
    chk_off.push_back((uint32_t)chk_inst.size());
    chk_probe.insert(chk_probe.end(), in[k].pose, in[k].pose + 3);
    chk_probe.insert(chk_probe.end(), in[k].odom_vel, in[k].odom_vel + 3);
    chk_probe.insert(chk_probe.end(), vs, vs + 3);
  }
  if (!chk_inst.empty()) {
    std::vector<double> cost(chk_inst.size(), -1.0);
    std::vector<int32_t> okc(chk_inst.size(), 0);
    const int rc = navgpu_tp_score_trajectories(f, (uint32_t)chk_inst.size(), chk_inst.data(), chk_off.data(), chk_probe.data(), cost.data(), okc.data());
    if (rc != NAVGPU_OK) return rc;
    for (size_t q = 0; q < chk_inst.size(); ++q) {
      if (!okc[q]) continue;  // zeros, false (:306-309, :350-351)
      navgpu_cmd_result& o = out[chk_k[q]];
      o.cmd_vel[0] = chk_probe[9 * q + 6];
      o.cmd_vel[1] = chk_probe[9 * q + 7];
      o.cmd_vel[2] = chk_probe[9 * q + 8];
      o.ok = 1;
    }
  }
  // --- the others drive (:489-525)
  for (uint32_t k = 0; k < count; ++k) {
    if (kind[k] != ROLLOUT) continue;
    navgpu_cmd_result& o = out[k];
    o.branch = NAVGPU_BRANCH_ROLLOUT;
    o.cmd_vel[0] = res[k].drive[0];
    o.cmd_vel[1] = res[k].drive[1];
    o.cmd_vel[2] = res[k].drive[2];
    o.ok = res[k].cost >= 0 ? 1 : 0;  // path.cost_ < 0: "failed to find a valid plan" (:495-502)
    o.trajectory_points = o.ok ? res[k].n_points : 0;
  }
  return NAVGPU_OK;
}

int navgpu_tp_ros_check_trajectories(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances, const navgpu_robot_input* in,
                                     const uint32_t* probe_offsets, const double* vel_samples, int32_t update_map, double* costs, int32_t* ok) {
  if (!f || !probe_offsets || (n_robots && (!instances || !in)) || n_robots > f->desc.n_instances || probe_offsets[0] != 0) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < n_robots; ++k)
    if (instances[k] >= f->desc.n_instances || (k && instances[k] <= instances[k - 1]) || probe_offsets[k + 1] < probe_offsets[k])
      return NAVGPU_ERR_INVALID;
  const uint32_t total = probe_offsets[n_robots];
  if (total && (!vel_samples || !costs)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->tpr_configured || !f->tp_configured) return NAVGPU_ERR_STATE;
  auto probed = [&](uint32_t k) { return in[k].have_pose && probe_offsets[k + 1] > probe_offsets[k]; };
  if (update_map) {  // updatePlan({pose}, true) (:531-539, :563-571): the planner's plan and final goal become the robot's pose
    std::vector<double> xy;   // one listed updatePlan for the probed robots, however they lie
    std::vector<uint32_t> who, off(1, 0u);
    for (uint32_t k = 0; k < n_robots; ++k) {
      if (!probed(k)) continue;
      who.push_back(instances[k]);
      xy.push_back(in[k].pose[0]);
      xy.push_back(in[k].pose[1]);
      off.push_back((uint32_t)who.size());
    }
    const int rc = navgpu_tp_update_plans_list(f, (uint32_t)who.size(), who.data(), xy.data(), off.data(), 1);
    if (rc != NAVGPU_OK) return rc;
  }
  std::vector<uint32_t> inst, off(1, 0u), where;  // where: the caller's index of each probe sent
  std::vector<double> probes;
  for (uint32_t k = 0; k < n_robots; ++k) {
    for (uint32_t p = probe_offsets[k]; p < probe_offsets[k + 1]; ++p) {  // "Failed to get the pose of the robot" (:554-555, :586-587)
      costs[p] = -1.0;
      if (ok) ok[p] = 0;
    }
    if (!probed(k)) continue;
    inst.push_back(instances[k]);
    for (uint32_t p = probe_offsets[k]; p < probe_offsets[k + 1]; ++p) {
      probes.insert(probes.end(), in[k].pose, in[k].pose + 3);
      probes.insert(probes.end(), in[k].odom_vel, in[k].odom_vel + 3);
      probes.insert(probes.end(), vel_samples + 3 * (size_t)p, vel_samples + 3 * (size_t)p + 3);
      where.push_back(p);
    }
    off.push_back((uint32_t)where.size());
  }
  if (where.empty()) return NAVGPU_OK;
  std::vector<double> c(where.size(), -1.0);
  std::vector<int32_t> o(where.size(), 0);
  const int rc = navgpu_tp_score_trajectories(f, (uint32_t)inst.size(), inst.data(), off.data(), probes.data(), c.data(), o.data());
  if (rc != NAVGPU_OK) return rc;
  for (size_t q = 0; q < where.size(); ++q) {
    costs[where[q]] = c[q];
    if (ok) ok[where[q]] = o[q];
  }
  return NAVGPU_OK;
}

}  // extern "C"
