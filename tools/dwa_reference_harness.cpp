// Runs DWA planning cycles through the reference's own classes, compiled in place by tools/make_dwa_goldens.py, and writes what they
// compute.  Nothing of the project (oracle or kernels) is linked.
//
// Two wirings:
//   planner (mode 0)  dwa_local_planner::DWAPlanner itself (dwa_planner.cpp, with local_planner_util.cpp and goal_functions.cpp), driven
//                     through reconfigure, setPlan, updatePlanAndLocalCosts, findBestPath and checkTrajectory: critic order, scales, the
//                     forward point and cheat_factor are the reference's.  DWAPlanner never passes discretize_by_time, an aggregation
//                     type or a yshift, so such cases cannot take this wiring.
//   direct  (mode 1)  the same generator, six critics and SimpleScoredSamplingPlanner, wired here as dwa_planner.cpp:57-81 (parameters
//                     and scales), :116-127,167-179 (construction, critic order), :240-286 (updatePlanAndLocalCosts), :298-319,357-368
//                     (findBestPath) and :217-230 (checkTrajectory) wire them, plus the three constructor / initialise arguments above.
// Every planner case is also run through the direct wiring and the two outputs are compared double for double; a difference is exit 4.
//
// The per-slot records need the planner's private critics and its generator's sample list.  The reference headers are therefore included
// with private and protected opened; the reference's sources are compiled unchanged (the Itanium C++ ABI lays classes out the same way
// whatever the access of their members).  After findBestPath the recorder restores the oscillation critic to its state before the cycle,
// re-initialises the generator with findBestPath's own arguments and asks the planner's SimpleScoredSamplingPlanner for all_explored
// (which findBestPath keeps in a local); the winner it reports must equal the one findBestPath returned (exit 5 otherwise).
//
// in : int64 n_cases; per case: int64 n_d, n_d doubles, int64 n_b, n_b map bytes (row-major, y first).  The doubles:
//      mode, size_x, size_y, resolution, n_fp, n_cycles, n_check, 22 configuration doubles and 8 ints in navgpu_dwa_config order,
//      aggregation[path, goal, goal_front, alignment], yshift[same], n_fp x {x, y}, per cycle {set_plan, pos[3], vel[3], n_plan,
//      n_plan x {x, y}}, n_check x sample[3].  Poses, velocities and samples are float32 values.
//      After the cases: int64 n_probe, n_probe x {pos[3], vel[3], dt} for SimpleTrajectoryGenerator::computeNewPositions.
// out: per case: int64 n, n doubles (see record() and main()); then n_probe x new_pos[3].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

// the standard library and the stand-ins first, so that only the reference's own headers see the opened access
#include <algorithm>
#include <list>
#include <map>
#include <queue>
#include <set>
#include <sstream>
#include <string>
#include <Eigen/Core>
#include <boost/thread.hpp>
#include <ros/ros.h>
#include <tf/transform_listener.h>
#include <pcl_ros/publisher.h>
#include <angles/angles.h>
#include <nav_msgs/Odometry.h>
#include <nav_msgs/Path.h>
#include <geometry_msgs/PolygonStamped.h>
#include <geometry_msgs/Twist.h>
#include <dwa_local_planner/DWAPlannerConfig.h>

#define private public
#define protected public
#include <dwa_local_planner/dwa_planner.h>
#include <base_local_planner/goal_functions.h>
#undef private
#undef protected

namespace blp = base_local_planner;
typedef Eigen::Vector3f V3;
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

struct Config {
  double d[22];  // navgpu_dwa_config's doubles, in its order
  int vx, vy, vth, use_dwa, discretize_by_time, sum_scores, allow_unknown;
  int agg[4];
  double yshift[4];
  double max_trans_vel() const { return d[0]; }
  double sim_time() const { return d[11]; }
  double sim_granularity() const { return d[12]; }
  double angular_sim_granularity() const { return d[13]; }
  double sim_period() const { return d[14]; }
  double path_distance_bias() const { return d[15]; }
  double goal_distance_bias() const { return d[16]; }
  double occdist_scale() const { return d[17]; }
  double forward_point_distance() const { return d[18]; }
  double cheat_factor() const { return d[19]; }
  double oscillation_reset_dist() const { return d[20]; }
  double oscillation_reset_angle() const { return d[21]; }
  blp::LocalPlannerLimits limits() const {
    blp::LocalPlannerLimits l(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], /*acc_limit_trans*/ 0.1,
                              /*xy_goal_tolerance*/ 0.1, /*yaw_goal_tolerance*/ 0.1);
    l.restore_defaults = false;
    return l;
  }
};

// What the recorder needs of either wiring.
struct Wiring {
  blp::SimpleTrajectoryGenerator* generator;
  blp::OscillationCostFunction* oscillation;
  blp::ObstacleCostFunction* obstacle;
  blp::MapGridCostFunction *goal_front, *alignment, *path, *goal;
  blp::SimpleScoredSamplingPlanner* sampler;
  blp::TrajectoryCostFunction* critic(int i) {
    blp::TrajectoryCostFunction* c[6] = {oscillation, obstacle, goal_front, alignment, path, goal};  // dwa_planner.cpp:168-173
    return c[i];
  }
};

static tf::Stamped<tf::Pose> stamped(const double* xyyaw) {
  tf::Stamped<tf::Pose> p;
  p.setOrigin(tf::Vector3(xyyaw[0], xyyaw[1], 0.0));
  p.setRotation(tf::createQuaternionFromYaw(xyyaw[2]));
  p.frame_id_ = "odom";
  return p;
}

static std::vector<geometry_msgs::PoseStamped> plan_msgs(const double* xy, int n) {
  std::vector<geometry_msgs::PoseStamped> plan(n);
  for (int i = 0; i < n; ++i) {
    plan[i].header.frame_id = "odom";
    plan[i].pose.position.x = xy[2 * i];
    plan[i].pose.position.y = xy[2 * i + 1];
  }
  return plan;
}

static bool same_trajectory(blp::Trajectory& a, blp::Trajectory& b) {
  if (a.cost_ < 0 && b.cost_ < 0) return true;  // no winner: findBestTrajectory leaves the rest of its argument as it was
  if (a.xv_ != b.xv_ || a.yv_ != b.yv_ || a.thetav_ != b.thetav_ || a.cost_ != b.cost_ || a.getPointsSize() != b.getPointsSize()) return false;
  for (unsigned i = 0; i < a.getPointsSize(); ++i) {
    double ax, ay, at, bx, by, bt;
    a.getPoint(i, ax, ay, at);
    b.getPoint(i, bx, by, bt);
    if (ax != bx || ay != by || at != bt) return false;
  }
  return true;
}

static uint32_t pack_flags(const blp::OscillationCostFunction& o) {  // bit order of navgpu_plan_result::oscillation_flags
  return (o.strafe_pos_only_ << 0) | (o.strafe_neg_only_ << 1) | (o.strafing_pos_ << 2) | (o.strafing_neg_ << 3) | (o.rot_pos_only_ << 4) |
         (o.rot_neg_only_ << 5) | (o.rotating_pos_ << 6) | (o.rotating_neg_ << 7) | (o.forward_pos_only_ << 8) | (o.forward_neg_only_ << 9) |
         (o.forward_pos_ << 10) | (o.forward_neg_ << 11);
}

// One cycle's record.  `before` is the oscillation critic as the cycle found it, `result` / `drive` what findBestPath returned.
//   pos[3], vel[3] (the floats the planner derived), scale[6], n_slots, per slot {sample[3], accepted, n_points, traj velocities[3],
//   raw critic[6], total without early-out, total in all_explored}, winner {found, slot, xv, yv, thetav, cost, n_points, points},
//   drive[3], flags, prev_stationary_pos[3], grids path / goal / goal_front (size_y x size_x each).
static int record(Wiring w, const blp::OscillationCostFunction& before, const V3& pos, const V3& vel, const V3& goal,
                  blp::LocalPlannerLimits limits, const V3& vsamples, int discretize_by_time, blp::Trajectory& result, const double* drive,
                  costmap_2d::Costmap2D& cm, std::vector<double>& out) {
  const blp::OscillationCostFunction after = *w.oscillation;
  *w.oscillation = before;
  if (discretize_by_time)
    w.generator->initialise(pos, vel, goal, &limits, vsamples, true);
  else
    w.generator->initialise(pos, vel, goal, &limits, vsamples);
  blp::Trajectory again;
  again.cost_ = -7;
  std::vector<blp::Trajectory> explored;
  w.sampler->findBestTrajectory(again, &explored);
  if (!same_trajectory(again, result)) return 5;
  for (int i = 0; i < 3; ++i) out.push_back(pos[i]);
  for (int i = 0; i < 3; ++i) out.push_back(vel[i]);
  for (int i = 0; i < 6; ++i) out.push_back(w.critic(i)->getScale());
  const std::vector<V3>& samples = w.generator->sample_params_;
  out.push_back((double)samples.size());
  size_t at = 0;
  int winner = -1;
  for (size_t s = 0; s < samples.size(); ++s) {
    blp::Trajectory t;
    const bool ok = w.generator->generateTrajectory(w.generator->pos_, w.generator->vel_, samples[s], t);
    for (int i = 0; i < 3; ++i) out.push_back(samples[s][i]);
    out.push_back(ok ? 1.0 : 0.0);
    if (!ok) {
      for (int i = 0; i < 12; ++i) out.push_back(kNaN);
      continue;
    }
    out.push_back((double)t.getPointsSize());
    out.push_back(t.xv_);
    out.push_back(t.yv_);
    out.push_back(t.thetav_);
    for (int i = 0; i < 6; ++i) out.push_back(w.critic(i)->scoreTrajectory(t));
    out.push_back(w.sampler->scoreTrajectory(t, -1));
    if (at >= explored.size()) return 6;
    out.push_back(explored[at].cost_);
    if (winner < 0 && result.cost_ >= 0 && same_trajectory(explored[at], result)) winner = (int)s;
    ++at;
  }
  if (at != explored.size()) return 6;
  out.push_back(result.cost_ >= 0 ? 1.0 : 0.0);
  out.push_back((double)winner);
  out.push_back(result.xv_);
  out.push_back(result.yv_);
  out.push_back(result.thetav_);
  out.push_back(result.cost_);
  const unsigned n_points = result.cost_ >= 0 ? result.getPointsSize() : 0;
  out.push_back((double)n_points);
  for (unsigned i = 0; i < n_points; ++i) {
    double x, y, th;
    result.getPoint(i, x, y, th);
    out.push_back(x);
    out.push_back(y);
    out.push_back(th);
  }
  for (int i = 0; i < 3; ++i) out.push_back(drive[i]);
  *w.oscillation = after;
  out.push_back((double)pack_flags(after));
  for (int i = 0; i < 3; ++i) out.push_back(after.prev_stationary_pos_[i]);
  blp::MapGridCostFunction* grids[3] = {w.path, w.goal, w.goal_front};
  for (int g = 0; g < 3; ++g)
    for (unsigned y = 0; y < cm.getSizeInCellsY(); ++y)
      for (unsigned x = 0; x < cm.getSizeInCellsX(); ++x) out.push_back(grids[g]->getCellCosts(x, y));
  return 0;
}

static void drive_of(tf::Stamped<tf::Pose>& d, double* out) {
  out[0] = d.getOrigin().getX();
  out[1] = d.getOrigin().getY();
  out[2] = tf::getYaw(d.getRotation());
}

// The direct wiring: the lines of dwa_planner.cpp named at the top of this file, with the arguments DWAPlanner leaves at their defaults.
struct Direct {
  const Config& c;
  costmap_2d::Costmap2D* cm;
  blp::SimpleTrajectoryGenerator generator;
  blp::OscillationCostFunction oscillation;
  blp::ObstacleCostFunction obstacle;
  blp::MapGridCostFunction path, goal, goal_front, alignment;
  blp::SimpleScoredSamplingPlanner sampler;
  std::vector<geometry_msgs::PoseStamped> global_plan;
  blp::Trajectory result;
  V3 vsamples;
  blp::LocalPlannerLimits limits;
  static blp::CostAggregationType agg(int a) { return a == 1 ? blp::Sum : a == 2 ? blp::Product : blp::Last; }
  Direct(const Config& cfg, costmap_2d::Costmap2D* costmap)
      : c(cfg), cm(costmap), obstacle(costmap), path(costmap, 0.0, cfg.yshift[0], false, agg(cfg.agg[0])),
        goal(costmap, 0.0, cfg.yshift[1], true, agg(cfg.agg[1])), goal_front(costmap, 0.0, cfg.yshift[2], true, agg(cfg.agg[2])),
        alignment(costmap, 0.0, cfg.yshift[3], false, agg(cfg.agg[3])), limits(cfg.limits()) {
    goal_front.setStopOnFailure(false);
    alignment.setStopOnFailure(false);
    oscillation.resetOscillationFlags();
    obstacle.setSumScores(c.sum_scores != 0);
    std::vector<blp::TrajectoryCostFunction*> critics;
    critics.push_back(&oscillation);
    critics.push_back(&obstacle);
    critics.push_back(&goal_front);
    critics.push_back(&alignment);
    critics.push_back(&path);
    critics.push_back(&goal);
    std::vector<blp::TrajectorySampleGenerator*> generators;
    generators.push_back(&generator);
    sampler = blp::SimpleScoredSamplingPlanner(generators, critics);
    // reconfigure
    generator.setParameters(c.sim_time(), c.sim_granularity(), c.angular_sim_granularity(), c.use_dwa != 0, c.sim_period());
    const double resolution = cm->getResolution();
    path.setScale(resolution * c.path_distance_bias() * 0.5);
    alignment.setScale(resolution * c.path_distance_bias() * 0.5);
    goal.setScale(resolution * c.goal_distance_bias() * 0.5);
    goal_front.setScale(resolution * c.goal_distance_bias() * 0.5);
    obstacle.setScale(resolution * c.occdist_scale());
    oscillation.setOscillationResetDist(c.oscillation_reset_dist(), c.oscillation_reset_angle());
    goal_front.setXShift(c.forward_point_distance());
    alignment.setXShift(c.forward_point_distance());
    obstacle.setParams(c.max_trans_vel(), 0.2, 0.25);
    vsamples[0] = c.vx <= 0 ? 1 : c.vx;
    vsamples[1] = c.vy <= 0 ? 1 : c.vy;
    vsamples[2] = c.vth <= 0 ? 1 : c.vth;
  }
  Wiring wiring() {
    Wiring w = {&generator, &oscillation, &obstacle, &goal_front, &alignment, &path, &goal, &sampler};
    return w;
  }
  void setPlan() { oscillation.resetOscillationFlags(); }
  void updatePlanAndLocalCosts(tf::Stamped<tf::Pose> global_pose, const std::vector<geometry_msgs::PoseStamped>& new_plan) {
    global_plan = new_plan;
    path.setTargetPoses(global_plan);
    goal.setTargetPoses(global_plan);
    geometry_msgs::PoseStamped goal_pose = global_plan.back();
    V3 pos(global_pose.getOrigin().getX(), global_pose.getOrigin().getY(), tf::getYaw(global_pose.getRotation()));
    double sq_dist = (pos[0] - goal_pose.pose.position.x) * (pos[0] - goal_pose.pose.position.x) +
                     (pos[1] - goal_pose.pose.position.y) * (pos[1] - goal_pose.pose.position.y);
    std::vector<geometry_msgs::PoseStamped> front = global_plan;
    double angle_to_goal = atan2(goal_pose.pose.position.y - pos[1], goal_pose.pose.position.x - pos[0]);
    front.back().pose.position.x = front.back().pose.position.x + c.forward_point_distance() * cos(angle_to_goal);
    front.back().pose.position.y = front.back().pose.position.y + c.forward_point_distance() * sin(angle_to_goal);
    goal_front.setTargetPoses(front);
    if (sq_dist > c.forward_point_distance() * c.forward_point_distance() * c.cheat_factor()) {
      alignment.setScale(cm->getResolution() * c.path_distance_bias() * 0.5);
      alignment.setTargetPoses(global_plan);
    } else {
      alignment.setScale(0.0);
    }
  }
  void poses(tf::Stamped<tf::Pose>& global_pose, tf::Stamped<tf::Pose>& global_vel, V3& pos, V3& vel, V3& goal_v) {
    pos = V3(global_pose.getOrigin().getX(), global_pose.getOrigin().getY(), tf::getYaw(global_pose.getRotation()));
    vel = V3(global_vel.getOrigin().getX(), global_vel.getOrigin().getY(), tf::getYaw(global_vel.getRotation()));
    geometry_msgs::PoseStamped goal_pose = global_plan.back();
    goal_v = V3(goal_pose.pose.position.x, goal_pose.pose.position.y, tf::getYaw(goal_pose.pose.orientation));
  }
  void initialise(const V3& pos, const V3& vel, const V3& goal_v) {
    if (c.discretize_by_time)
      generator.initialise(pos, vel, goal_v, &limits, vsamples, true);
    else
      generator.initialise(pos, vel, goal_v, &limits, vsamples);
  }
  blp::Trajectory findBestPath(tf::Stamped<tf::Pose> global_pose, tf::Stamped<tf::Pose> global_vel, tf::Stamped<tf::Pose>& drive,
                               std::vector<geometry_msgs::Point> footprint) {
    obstacle.setFootprint(footprint);
    V3 pos, vel, goal_v;
    poses(global_pose, global_vel, pos, vel, goal_v);
    initialise(pos, vel, goal_v);
    result.cost_ = -7;
    std::vector<blp::Trajectory> all_explored;
    sampler.findBestTrajectory(result, &all_explored);
    oscillation.updateOscillationFlags(pos, &result, limits.min_trans_vel);
    if (result.cost_ < 0) {
      drive.setIdentity();
    } else {
      drive.setOrigin(tf::Vector3(result.xv_, result.yv_, 0));
      tf::Matrix3x3 matrix;
      matrix.setRotation(tf::createQuaternionFromYaw(result.thetav_));
      drive.setBasis(matrix);
    }
    return result;
  }
  bool checkTrajectory(V3 pos, V3 vel, V3 vel_samples) {
    oscillation.resetOscillationFlags();
    blp::Trajectory traj;
    geometry_msgs::PoseStamped goal_pose = global_plan.back();
    V3 goal_v(goal_pose.pose.position.x, goal_pose.pose.position.y, tf::getYaw(goal_pose.pose.orientation));
    initialise(pos, vel, goal_v);
    generator.generateTrajectory(pos, vel, vel_samples, traj);
    return sampler.scoreTrajectory(traj, -1) >= 0;
  }
};

struct Case {
  int mode, size_x, size_y, n_fp, n_cycles, n_check;
  double resolution;
  Config cfg;
  std::vector<geometry_msgs::Point> footprint;
  const double* cycles;
  const double* checks;
  const uint8_t* map;
};

// Runs one case through wiring P (DWAPlanner or Direct) with `make` building it.
template <class Run>
static int run_case(const Case& k, Run& p, Wiring w, costmap_2d::Costmap2D& cm, std::vector<double>& out) {
  const double* at = k.cycles;
  double last_pos[3] = {0, 0, 0}, last_vel[3] = {0, 0, 0};
  for (int cyc = 0; cyc < k.n_cycles; ++cyc) {
    const int set_plan = (int)at[0];
    const double *pos_in = at + 1, *vel_in = at + 4;
    const int n_plan = (int)at[7];
    std::vector<geometry_msgs::PoseStamped> plan = plan_msgs(at + 8, n_plan);
    at += 8 + 2 * n_plan;
    tf::Stamped<tf::Pose> pose = stamped(pos_in), velocity = stamped(vel_in), drive;
    if (set_plan) p.setPlan(plan);
    p.updatePlanAndLocalCosts(pose, plan);
    const blp::OscillationCostFunction before = *w.oscillation;
    blp::Trajectory result = p.findBestPath(pose, velocity, drive, k.footprint);
    double d[3];
    drive_of(drive, d);
    V3 pos(pose.getOrigin().getX(), pose.getOrigin().getY(), tf::getYaw(pose.getRotation()));
    V3 vel(velocity.getOrigin().getX(), velocity.getOrigin().getY(), tf::getYaw(velocity.getRotation()));
    V3 goal(plan.back().pose.position.x, plan.back().pose.position.y, tf::getYaw(plan.back().pose.orientation));
    V3 vsamples;
    vsamples[0] = k.cfg.vx <= 0 ? 1 : k.cfg.vx;
    vsamples[1] = k.cfg.vy <= 0 ? 1 : k.cfg.vy;
    vsamples[2] = k.cfg.vth <= 0 ? 1 : k.cfg.vth;
    int rc = record(w, before, pos, vel, goal, k.cfg.limits(), vsamples, k.cfg.discretize_by_time, result, d, cm, out);
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) last_pos[i] = pos_in[i], last_vel[i] = vel_in[i];
  }
  for (int i = 0; i < k.n_check; ++i) {
    const double* s = k.checks + 3 * i;
    V3 pos(last_pos[0], last_pos[1], last_pos[2]), vel(last_vel[0], last_vel[1], last_vel[2]), sample(s[0], s[1], s[2]);
    out.push_back(p.checkTrajectory(pos, vel, sample) ? 1.0 : 0.0);
  }
  return 0;
}

struct PlannerRun {  // DWAPlanner behind the calls run_case makes
  dwa_local_planner::DWAPlanner& dp;
  void setPlan(const std::vector<geometry_msgs::PoseStamped>& plan) { dp.setPlan(plan); }
  void updatePlanAndLocalCosts(tf::Stamped<tf::Pose> pose, const std::vector<geometry_msgs::PoseStamped>& plan) { dp.updatePlanAndLocalCosts(pose, plan); }
  blp::Trajectory findBestPath(tf::Stamped<tf::Pose> pose, tf::Stamped<tf::Pose> vel, tf::Stamped<tf::Pose>& drive, std::vector<geometry_msgs::Point> fp) {
    return dp.findBestPath(pose, vel, drive, fp);
  }
  bool checkTrajectory(V3 pos, V3 vel, V3 sample) { return dp.checkTrajectory(pos, vel, sample); }
};

struct DirectRun {
  Direct& d;
  void setPlan(const std::vector<geometry_msgs::PoseStamped>&) { d.setPlan(); }
  void updatePlanAndLocalCosts(tf::Stamped<tf::Pose> pose, const std::vector<geometry_msgs::PoseStamped>& plan) { d.updatePlanAndLocalCosts(pose, plan); }
  blp::Trajectory findBestPath(tf::Stamped<tf::Pose> pose, tf::Stamped<tf::Pose> vel, tf::Stamped<tf::Pose>& drive, std::vector<geometry_msgs::Point> fp) {
    return d.findBestPath(pose, vel, drive, fp);
  }
  bool checkTrajectory(V3 pos, V3 vel, V3 sample) { return d.checkTrajectory(pos, vel, sample); }
};

static void fill_costmap(costmap_2d::Costmap2D& cm, const Case& k) {
  for (int y = 0; y < k.size_y; ++y)
    for (int x = 0; x < k.size_x; ++x) cm.setCost(x, y, k.map[(size_t)y * k.size_x + x]);
}

static int run_direct(const Case& k, std::vector<double>& out) {
  costmap_2d::Costmap2D cm(k.size_x, k.size_y, k.resolution, 0.0, 0.0, k.cfg.allow_unknown ? 255 : 0);
  fill_costmap(cm, k);
  Direct d(k.cfg, &cm);
  // The reference reads allow_unknown from a Costmap2D copy whose default_value_ the copy never sets (costmap_model.cpp:47,
  // map_grid.cpp:106): what it does with NO_INFORMATION cells is not defined, so maps that hold any are refused.
  for (int i = 0; i < k.size_x * k.size_y; ++i)
    if (k.map[i] == costmap_2d::NO_INFORMATION) return 8;
  DirectRun r = {d};
  return run_case(k, r, d.wiring(), cm, out);
}

static int run_planner(const Case& k, std::vector<double>& out) {
  costmap_2d::Costmap2D cm(k.size_x, k.size_y, k.resolution, 0.0, 0.0, k.cfg.allow_unknown ? 255 : 0);
  fill_costmap(cm, k);
  dwa_ref::params().clear();
  dwa_ref::params()["sum_scores"] = k.cfg.sum_scores;
  dwa_ref::params()["cheat_factor"] = k.cfg.cheat_factor();
  if (k.cfg.sim_period() != 0.05) return 7;  // the constructor derives it from controller_frequency; the cases keep its default
  tf::TransformListener listener;
  blp::LocalPlannerUtil util;
  util.initialize(&listener, &cm, "odom");
  blp::LocalPlannerLimits limits = k.cfg.limits();
  util.reconfigureCB(limits, false);
  dwa_local_planner::DWAPlanner dp("dwa", &util);
  dwa_local_planner::DWAPlannerConfig c;
  c.sim_time = k.cfg.sim_time();
  c.sim_granularity = k.cfg.sim_granularity();
  c.angular_sim_granularity = k.cfg.angular_sim_granularity();
  c.use_dwa = k.cfg.use_dwa != 0;
  c.path_distance_bias = k.cfg.path_distance_bias();
  c.goal_distance_bias = k.cfg.goal_distance_bias();
  c.occdist_scale = k.cfg.occdist_scale();
  c.stop_time_buffer = 0.2;
  c.oscillation_reset_dist = k.cfg.oscillation_reset_dist();
  c.oscillation_reset_angle = k.cfg.oscillation_reset_angle();
  c.forward_point_distance = k.cfg.forward_point_distance();
  c.max_trans_vel = k.cfg.max_trans_vel();
  c.max_scaling_factor = 0.2;
  c.scaling_speed = 0.25;
  c.vx_samples = k.cfg.vx;
  c.vy_samples = k.cfg.vy;
  c.vth_samples = k.cfg.vth;
  dp.reconfigure(c);
  Wiring w = {&dp.generator_, &dp.oscillation_costs_, &dp.obstacle_costs_, &dp.goal_front_costs_, &dp.alignment_costs_, &dp.path_costs_,
              &dp.goal_costs_, &dp.scored_sampling_planner_};
  PlannerRun r = {dp};
  return run_case(k, r, w, cm, out);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, sizeof n_cases, 1, in) != 1) return 3;
  for (int64_t ci = 0; ci < n_cases; ++ci) {
    int64_t n_d = 0, n_b = 0;
    if (fread(&n_d, sizeof n_d, 1, in) != 1) return 3;
    std::vector<double> d(n_d);
    if (fread(d.data(), sizeof(double), n_d, in) != (size_t)n_d) return 3;
    if (fread(&n_b, sizeof n_b, 1, in) != 1) return 3;
    std::vector<uint8_t> map(n_b);
    if (fread(map.data(), 1, n_b, in) != (size_t)n_b) return 3;
    Case k;
    k.mode = (int)d[0], k.size_x = (int)d[1], k.size_y = (int)d[2], k.resolution = d[3];
    k.n_fp = (int)d[4], k.n_cycles = (int)d[5], k.n_check = (int)d[6];
    if ((int64_t)k.size_x * k.size_y != n_b) return 3;
    for (int i = 0; i < 22; ++i) k.cfg.d[i] = d[7 + i];
    k.cfg.vx = (int)d[29], k.cfg.vy = (int)d[30], k.cfg.vth = (int)d[31], k.cfg.use_dwa = (int)d[32];
    k.cfg.discretize_by_time = (int)d[33], k.cfg.sum_scores = (int)d[34], k.cfg.allow_unknown = (int)d[35];
    for (int i = 0; i < 4; ++i) k.cfg.agg[i] = (int)d[37 + i], k.cfg.yshift[i] = d[41 + i];
    const double* at = d.data() + 45;
    for (int i = 0; i < k.n_fp; ++i) {
      geometry_msgs::Point p;
      p.x = at[2 * i], p.y = at[2 * i + 1], p.z = 0;
      k.footprint.push_back(p);
    }
    at += 2 * k.n_fp;
    k.cycles = at;
    for (int c = 0; c < k.n_cycles; ++c) at += 8 + 2 * (int)at[7];
    k.checks = at;
    if (at + 3 * k.n_check != d.data() + n_d) return 3;
    k.map = map.data();
    std::vector<double> res;
    int rc = run_direct(k, res);
    if (rc) return rc;
    if (k.mode == 0) {
      if (k.cfg.discretize_by_time) return 7;
      for (int i = 0; i < 4; ++i)
        if (k.cfg.agg[i] || k.cfg.yshift[i] != 0.0) return 7;
      std::vector<double> own;
      rc = run_planner(k, own);
      if (rc) return rc;
      if (own.size() != res.size() || memcmp(own.data(), res.data(), own.size() * sizeof(double)) != 0) {
        fprintf(stderr, "case %lld: DWAPlanner and the direct wiring differ\n", (long long)ci);
        return 4;
      }
      res.swap(own);
    }
    const int64_t n = (int64_t)res.size();
    fwrite(&n, sizeof n, 1, out);
    fwrite(res.data(), sizeof(double), res.size(), out);
  }
  // which cos / sin the rollout was compiled with: computeNewPositions itself on the probe states that follow the cases
  int64_t n_probe = 0;
  if (fread(&n_probe, sizeof n_probe, 1, in) != 1) return 3;
  for (int64_t i = 0; i < n_probe; ++i) {
    double q[7];
    if (fread(q, sizeof(double), 7, in) != 7) return 3;
    const V3 next = blp::SimpleTrajectoryGenerator::computeNewPositions(V3(q[0], q[1], q[2]), V3(q[3], q[4], q[5]), q[6]);
    const double r[3] = {next[0], next[1], next[2]};
    fwrite(r, sizeof(double), 3, out);
  }
  fclose(out);
  fclose(in);
  return 0;
}
