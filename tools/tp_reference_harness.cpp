// Runs planning cycles through the reference's own base_local_planner::TrajectoryPlanner, compiled in place by tools/make_tp_goldens.py
// (with CostmapModel, MapGrid, MapCell, FootprintHelper, Trajectory, Costmap2D and costmap_2d/footprint.cpp), and writes what it
// computes.  Nothing of the project (oracle or library) is linked.
//
// How the generateTrajectory calls are observed (the function is called inside createTrajectories and cannot be subclassed):
//   * Trajectory::resetPoints() is wrapped at link time (-Wl,--wrap=<mangled name>).  generateTrajectory calls it on its output argument
//     before writing anything, so the wrapper learns which object (traj_one / traj_two, or scoreTrajectory's local) the call fills.
//   * the harness's boost::mutex stand-in (tools/tp_ref_stubs/boost/thread.hpp) reports every unlock.  generateTrajectory holds
//     configuration_mutex_ for its whole body, so at the unlock that object holds the call's sample, cost_ and points - before
//     createTrajectories can patch the backing-up call's -1 to 1.0.
//   The winner's call index is the last call that wrote the member whose contents equal the returned trajectory; a cycle where both
//   members equal it is refused (exit 5).
// The planner is given a WorldModel of the harness's own, a CostmapModel subclass that forwards: it sees every rollout position and
// oriented footprint vertex, of which only the distance to the nearest cell boundary is kept (the generator's knife-edge guard).
//
// The reference headers are included with private and protected opened (the sources are compiled unchanged; the Itanium C++ ABI lays
// classes out the same way whatever the access of their members).  meter_scoring_ is a member the reference's constructor never
// initialises (trajectory_planner.cpp:156-171 has no entry for it) and reconfigure reads (:84): the harness sets it from the case.
//
// in : int64 n_cases; per case: int64 n_d, n_d doubles, int64 n_b, n_b map bytes (row-major, y first).  The doubles:
//      size_x, size_y, resolution, origin_x, origin_y, default_value, n_fp, n_cycles, CFG, n_fp x {x, y}, then per cycle
//      {has_reconfigure, [CFG], n_plan (-1: keep the plan), compute_dists, n_plan x {x, y}, mode (0: pose given, 1: advanced from the
//      last command), pos[3], vel[3], dt, n_pre, n_pre x sample[3], n_post, n_post x sample[3]}.
//      CFG = 21 doubles in navgpu_tp_config order, vx_samples, vtheta_samples, holonomic_robot, dwa, heading_scoring, simple_attractor,
//      meter_scoring, n_y_vels, y_vels[8].
// out: per case: int64 n, n doubles: per cycle {CFG as read back from the object, pos[3], vel[3], n_pre, n_pre x cost, n_calls,
//      n_calls x {vx, vy, vtheta, cost, n_points, last point[3]}, winner {xv, yv, thetav, cost, n_points, call index}, points, drive[3], flags,
//      prev_x, prev_y, escape_x, escape_y, escape_theta, n_within, within cells, path grid, goal grid, n_post, n_post x {cost, check}},
//      then the smallest boundary distance (cells) and allow_unknown_ as the planner read it.
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
#include <boost/algorithm/string.hpp>
#include <ros/ros.h>
#include <tf/tf.h>
#include <angles/angles.h>
#include <geometry_msgs/PoseStamped.h>
#include <geometry_msgs/Point.h>
#include <base_local_planner/BaseLocalPlannerConfig.h>

#define private public
#define protected public
#include <base_local_planner/trajectory_planner.h>
#include <base_local_planner/costmap_model.h>
#undef private
#undef protected

namespace blp = base_local_planner;
static const int N_CFG = 37;

// ---- observation of the generateTrajectory calls
struct Call {
  const blp::Trajectory* object;
  double vx, vy, vth, cost;
  int n_points;
  double end[3];  // the last point (NaN without points)
};
static bool g_recording = false;
static const blp::Trajectory* g_pending = nullptr;
static std::vector<Call> g_calls;

extern "C" void __real__ZN18base_local_planner10Trajectory11resetPointsEv(blp::Trajectory* self);
extern "C" void __wrap__ZN18base_local_planner10Trajectory11resetPointsEv(blp::Trajectory* self) {
  if (g_recording) g_pending = self;
  __real__ZN18base_local_planner10Trajectory11resetPointsEv(self);
}
static void on_unlock() {
  if (!g_recording || !g_pending) return;
  const blp::Trajectory& t = *g_pending;
  Call k = {g_pending, t.xv_, t.yv_, t.thetav_, t.cost_, (int)t.x_pts_.size(), {NAN, NAN, NAN}};
  if (k.n_points) k.end[0] = t.x_pts_.back(), k.end[1] = t.y_pts_.back(), k.end[2] = t.th_pts_.back();
  g_calls.push_back(k);
  g_pending = nullptr;
}

// ---- the knife-edge guard's measurement
static double g_margin = 1e300;
struct WatchingModel : public blp::CostmapModel {
  const costmap_2d::Costmap2D& cm;
  explicit WatchingModel(const costmap_2d::Costmap2D& c) : blp::CostmapModel(c), cm(c) {}
  using blp::WorldModel::footprintCost;
  void see(double wx, double wy) {
    const double fx = (wx - cm.getOriginX()) / cm.getResolution(), fy = (wy - cm.getOriginY()) / cm.getResolution();
    g_margin = std::min(g_margin, std::min(fabs(fx - floor(fx + 0.5)), fabs(fy - floor(fy + 0.5))));
  }
  virtual double footprintCost(const geometry_msgs::Point& position, const std::vector<geometry_msgs::Point>& footprint,
                               double inscribed_radius, double circumscribed_radius) {
    see(position.x, position.y);
    for (size_t i = 0; i < footprint.size(); ++i) see(footprint[i].x, footprint[i].y);
    return blp::CostmapModel::footprintCost(position, footprint, inscribed_radius, circumscribed_radius);
  }
};

struct Cfg {
  double v[N_CFG];
  std::vector<double> y_vels() const { return std::vector<double>(v + 29, v + 29 + (int)v[28]); }
  blp::BaseLocalPlannerConfig message() const {
    blp::BaseLocalPlannerConfig c;
    c.acc_lim_x = v[0], c.acc_lim_y = v[1], c.acc_lim_theta = v[2], c.sim_time = v[3], c.sim_granularity = v[4];
    c.angular_sim_granularity = v[5], c.pdist_scale = v[6], c.gdist_scale = v[7], c.occdist_scale = v[8], c.heading_lookahead = v[9];
    c.oscillation_reset_dist = v[10], c.escape_reset_dist = v[11], c.escape_reset_theta = v[12], c.max_vel_x = v[13], c.min_vel_x = v[14];
    c.max_vel_theta = v[15], c.min_vel_theta = v[16], c.min_in_place_vel_theta = v[17], c.escape_vel = v[18];
    c.heading_scoring_timestep = v[20];
    c.vx_samples = (int)v[21], c.vtheta_samples = (int)v[22], c.holonomic_robot = v[23] != 0, c.dwa = v[24] != 0;
    c.heading_scoring = v[25] != 0, c.simple_attractor = v[26] != 0, c.restore_defaults = false;
    std::ostringstream s;
    s.precision(17);
    const std::vector<double> y = y_vels();
    for (size_t i = 0; i < y.size(); ++i) s << (i ? ", " : "") << y[i];
    c.y_vels = s.str();
    return c;
  }
};

static void read_back(const blp::TrajectoryPlanner& tp, std::vector<double>& out) {
  const double d[21] = {tp.acc_lim_x_, tp.acc_lim_y_, tp.acc_lim_theta_, tp.sim_time_, tp.sim_granularity_, tp.angular_sim_granularity_,
                        tp.pdist_scale_, tp.gdist_scale_, tp.occdist_scale_, tp.heading_lookahead_, tp.oscillation_reset_dist_,
                        tp.escape_reset_dist_, tp.escape_reset_theta_, tp.max_vel_x_, tp.min_vel_x_, tp.max_vel_th_, tp.min_vel_th_,
                        tp.min_in_place_vel_th_, tp.backup_vel_, tp.sim_period_, tp.heading_scoring_timestep_};
  out.insert(out.end(), d, d + 21);
  out.push_back(tp.vx_samples_);
  out.push_back(tp.vtheta_samples_);
  out.push_back(tp.holonomic_robot_);
  out.push_back(tp.dwa_);
  out.push_back(tp.heading_scoring_);
  out.push_back(tp.simple_attractor_);
  out.push_back(tp.meter_scoring_);
  out.push_back((double)tp.y_vels_.size());
  for (size_t i = 0; i < 8; ++i) out.push_back(i < tp.y_vels_.size() ? tp.y_vels_[i] : 0.0);
}

static tf::Stamped<tf::Pose> stamped(const float* xyyaw) {
  tf::Stamped<tf::Pose> p;
  p.setOrigin(tf::Vector3(xyyaw[0], xyyaw[1], 0.0));
  p.setRotation(tf::createQuaternionFromYaw(xyyaw[2]));
  p.frame_id_ = "odom";
  return p;
}

static bool same(const blp::Trajectory& a, const blp::Trajectory& b) {
  return a.xv_ == b.xv_ && a.yv_ == b.yv_ && a.thetav_ == b.thetav_ && a.cost_ == b.cost_ && a.x_pts_ == b.x_pts_ && a.y_pts_ == b.y_pts_ &&
         a.th_pts_ == b.th_pts_;
}

static int run_case(const std::vector<double>& d, const std::vector<uint8_t>& map, std::vector<double>& out) {
  const int size_x = (int)d[0], size_y = (int)d[1], n_fp = (int)d[6], n_cycles = (int)d[7];
  const double resolution = d[2];
  if ((size_t)size_x * size_y != map.size()) return 3;
  costmap_2d::Costmap2D cm(size_x, size_y, resolution, d[3], d[4], (unsigned char)d[5]);
  for (int y = 0; y < size_y; ++y)
    for (int x = 0; x < size_x; ++x) {
      // The reference takes allow_unknown from a Costmap2D copy whose default_value_ the copy never sets (trajectory_planner.cpp:186,
      // costmap_model.cpp:47, map_grid.cpp:106): what it does with NO_INFORMATION cells is not defined, so maps that hold any are refused.
      if (map[(size_t)y * size_x + x] == costmap_2d::NO_INFORMATION) return 8;
      cm.setCost(x, y, map[(size_t)y * size_x + x]);
    }
  Cfg c;
  memcpy(c.v, &d[8], sizeof c.v);
  const double* at = &d[8 + N_CFG];
  std::vector<geometry_msgs::Point> footprint(n_fp);
  for (int i = 0; i < n_fp; ++i) footprint[i].x = at[2 * i], footprint[i].y = at[2 * i + 1], footprint[i].z = 0;
  at += 2 * n_fp;
  WatchingModel wm(cm);
  blp::TrajectoryPlanner tp(wm, cm, footprint, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], (int)c.v[21], (int)c.v[22], c.v[6], c.v[7], c.v[8],
                            c.v[9], c.v[10], c.v[11], c.v[12], c.v[23] != 0, c.v[13], c.v[14], c.v[15], c.v[16], c.v[17], c.v[18], c.v[24] != 0,
                            c.v[25] != 0, c.v[20], c.v[27] != 0, c.v[26] != 0, c.y_vels(), /*stop_time_buffer*/ 0.2, c.v[19], c.v[5]);
  tp.meter_scoring_ = c.v[27] != 0;
  float pos[3] = {0, 0, 0}, vel[3] = {0, 0, 0};
  double command[3] = {0, 0, 0};
  g_margin = 1e300;
  for (int cyc = 0; cyc < n_cycles; ++cyc) {
    if (*at++ != 0.0) {
      Cfg r;
      memcpy(r.v, at, sizeof r.v);
      at += N_CFG;
      tp.meter_scoring_ = r.v[27] != 0;
      blp::BaseLocalPlannerConfig msg = r.message();
      tp.reconfigure(msg);
    }
    const int n_plan = (int)at[0];
    const bool compute_dists = at[1] != 0.0;
    at += 2;
    if (n_plan >= 0) {
      std::vector<geometry_msgs::PoseStamped> plan(n_plan);
      for (int i = 0; i < n_plan; ++i) {
        plan[i].header.frame_id = "odom";
        plan[i].pose.position.x = at[2 * i];
        plan[i].pose.position.y = at[2 * i + 1];
        plan[i].pose.orientation.w = 1.0;
      }
      at += 2 * n_plan;
      tp.updatePlan(plan, compute_dists);
    }
    const int mode = (int)at[0];
    const double dt = at[7];
    if (mode == 0) {
      for (int i = 0; i < 3; ++i) pos[i] = (float)at[1 + i], vel[i] = (float)at[4 + i];
    } else {  // the pose a robot obeying the last command for dt reaches; odometry reports the command
      const double th = pos[2];
      pos[0] = (float)((double)pos[0] + (command[0] * cos(th) - command[1] * sin(th)) * dt);
      pos[1] = (float)((double)pos[1] + (command[0] * sin(th) + command[1] * cos(th)) * dt);
      pos[2] = (float)(th + command[2] * dt);
      for (int i = 0; i < 3; ++i) vel[i] = (float)command[i];
    }
    at += 8;
    read_back(tp, out);
    for (int i = 0; i < 3; ++i) out.push_back(pos[i]);
    for (int i = 0; i < 3; ++i) out.push_back(vel[i]);
    const int n_pre = (int)*at++;
    out.push_back(n_pre);
    for (int i = 0; i < n_pre; ++i, at += 3) out.push_back(tp.scoreTrajectory(pos[0], pos[1], pos[2], vel[0], vel[1], vel[2], at[0], at[1], at[2]));
    // ---- the cycle
    tf::Stamped<tf::Pose> pose = stamped(pos), velocity = stamped(vel), drive;
    // the Eigen::Vector3f findBestPath derives (:911-912) must be the floats handed in: the fixture's pose is then what the planner used
    if ((float)tf::getYaw(pose.getRotation()) != pos[2] || (float)tf::getYaw(velocity.getRotation()) != vel[2]) return 6;
    g_calls.clear();
    g_pending = nullptr;
    g_recording = true;
    blp::Trajectory best = tp.findBestPath(pose, velocity, drive);
    g_recording = false;
    if (g_pending) return 7;
    int last_one = -1, last_two = -1;
    for (size_t i = 0; i < g_calls.size(); ++i) {
      if (g_calls[i].object == &tp.traj_one) last_one = (int)i;
      else if (g_calls[i].object == &tp.traj_two) last_two = (int)i;
      else return 7;
    }
    const bool is_one = last_one >= 0 && same(tp.traj_one, best), is_two = last_two >= 0 && same(tp.traj_two, best);
    if (is_one == is_two) {
      fprintf(stderr, "cycle %d: the returned trajectory equals %s of the planner's two members\n", cyc, is_one ? "both" : "neither");
      return 5;
    }
    out.push_back((double)g_calls.size());
    for (size_t i = 0; i < g_calls.size(); ++i) {
      const Call& k = g_calls[i];
      const double r[8] = {k.vx, k.vy, k.vth, k.cost, (double)k.n_points, k.end[0], k.end[1], k.end[2]};
      out.insert(out.end(), r, r + 8);
    }
    const double w[6] = {best.xv_, best.yv_, best.thetav_, best.cost_, (double)best.getPointsSize(), (double)(is_one ? last_one : last_two)};
    out.insert(out.end(), w, w + 6);
    for (unsigned i = 0; i < best.getPointsSize(); ++i) {
      double x, y, th;
      best.getPoint(i, x, y, th);
      out.push_back(x), out.push_back(y), out.push_back(th);
    }
    out.push_back(drive.getOrigin().getX());
    out.push_back(drive.getOrigin().getY());
    out.push_back(tf::getYaw(drive.getRotation()));
    const unsigned flags = (tp.stuck_left << 0) | (tp.stuck_right << 1) | (tp.rotating_left << 2) | (tp.rotating_right << 3) |
                           (tp.stuck_left_strafe << 4) | (tp.stuck_right_strafe << 5) | (tp.strafe_left << 6) | (tp.strafe_right << 7) |
                           (tp.escaping_ << 8);  // bit order of navgpu_tp_state::flags
    out.push_back((double)flags);
    out.push_back(tp.prev_x_), out.push_back(tp.prev_y_), out.push_back(tp.escape_x_), out.push_back(tp.escape_y_), out.push_back(tp.escape_theta_);
    std::vector<double> within;
    for (int y = 0; y < size_y; ++y)
      for (int x = 0; x < size_x; ++x)
        if (tp.path_map_(x, y).within_robot) within.push_back((double)(y * size_x + x));
    out.push_back((double)within.size());
    out.insert(out.end(), within.begin(), within.end());
    for (int g = 0; g < 2; ++g)
      for (int y = 0; y < size_y; ++y)
        for (int x = 0; x < size_x; ++x) out.push_back((g ? tp.goal_map_ : tp.path_map_)(x, y).target_dist);
    const int n_post = (int)*at++;
    out.push_back(n_post);
    for (int i = 0; i < n_post; ++i, at += 3) {
      out.push_back(tp.scoreTrajectory(pos[0], pos[1], pos[2], vel[0], vel[1], vel[2], at[0], at[1], at[2]));
      out.push_back(tp.checkTrajectory(pos[0], pos[1], pos[2], vel[0], vel[1], vel[2], at[0], at[1], at[2]) ? 1.0 : 0.0);
    }
    if (best.cost_ >= 0)
      command[0] = best.xv_, command[1] = best.yv_, command[2] = best.thetav_;
    else
      command[0] = command[1] = command[2] = 0.0;
  }
  if (at != d.data() + d.size()) return 3;
  out.push_back(g_margin);
  out.push_back(tp.allow_unknown_ ? 1.0 : 0.0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  tp_ref::unlock_hook() = on_unlock;
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
    std::vector<double> res;
    const int rc = run_case(d, map, res);
    if (rc) {
      fprintf(stderr, "case %lld: exit %d\n", (long long)ci, rc);
      return rc;
    }
    const int64_t n = (int64_t)res.size();
    fwrite(&n, sizeof n, 1, out);
    fwrite(res.data(), sizeof(double), res.size(), out);
  }
  fclose(out);
  fclose(in);
  return 0;
}
