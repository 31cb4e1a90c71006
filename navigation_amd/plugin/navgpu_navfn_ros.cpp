// navgpu::NavfnROS (navgpu_navfn_ros.h): navfn::NavfnROS's ROS face over the navgpu_navfn_ros_* calls.
#include "navgpu_navfn_ros.h"

#include <cfloat>

#include <boost/bind.hpp>
#include <pcl/point_cloud.h>
#include <pcl_conversions/pcl_conversions.h>
#include <pluginlib/class_list_macros.h>
#include <tf/tf.h>

PLUGINLIB_EXPORT_CLASS(navgpu::NavfnROS, nav_core::BaseGlobalPlanner)

namespace navgpu {

namespace {
// tf::resolve(prefix, frame_name) as tf documents it (tf is not part of the reference tree): an absolute name stays, a relative one
// goes under the prefix
std::string resolveFrame(const std::string& prefix, const std::string& frame_name) {
  if (!frame_name.empty() && frame_name[0] == '/') return frame_name;
  if (prefix.empty()) return "/" + frame_name;
  return (prefix[0] == '/' ? prefix : "/" + prefix) + "/" + frame_name;
}
const char* kNotInitialized = "This planner has not been initialized yet, but it is being used, please call initialize() before use";
}  // namespace

NavfnROS::NavfnROS()
    : costmap_(NULL), initialized_(false), allow_unknown_(true), visualize_potential_(false), planner_window_x_(0), planner_window_y_(0),
      default_tolerance_(0), params_(), handle_(NULL), nx_(0), ny_(0) {}

NavfnROS::NavfnROS(std::string name, costmap_2d::Costmap2DROS* costmap_ros)
    : costmap_(NULL), initialized_(false), allow_unknown_(true), visualize_potential_(false), planner_window_x_(0), planner_window_y_(0),
      default_tolerance_(0), params_(), handle_(NULL), nx_(0), ny_(0) {
  initialize(name, costmap_ros);
}

NavfnROS::NavfnROS(std::string name, costmap_2d::Costmap2D* costmap, std::string global_frame)
    : costmap_(NULL), initialized_(false), allow_unknown_(true), visualize_potential_(false), planner_window_x_(0), planner_window_y_(0),
      default_tolerance_(0), params_(), handle_(NULL), nx_(0), ny_(0) {
  initialize(name, costmap, global_frame);
}

NavfnROS::~NavfnROS() {
  if (handle_) navgpu_navfn_destroy(handle_);
}

void NavfnROS::initialize(std::string name, costmap_2d::Costmap2DROS* costmap_ros) {
  initialize(name, costmap_ros->getCostmap(), costmap_ros->getGlobalFrameID());
}

void NavfnROS::initialize(std::string name, costmap_2d::Costmap2D* costmap, std::string global_frame) {
  if (initialized_) {
    ROS_WARN("This planner has already been initialized, you can't call it twice, doing nothing");
    return;
  }
  costmap_ = costmap;
  global_frame_ = global_frame;
  ros::NodeHandle private_nh("~/" + name);
  plan_pub_ = private_nh.advertise<nav_msgs::Path>("plan", 1);
  private_nh.param("visualize_potential", visualize_potential_, false);
  if (visualize_potential_) potarr_pub_.advertise(private_nh, "potential", 1);
  private_nh.param("planner_window_x", planner_window_x_, 0.0);
  private_nh.param("planner_window_y", planner_window_y_, 0.0);
  bool wavefront;  // no counterpart in the reference: the expansion as the library's tiled wavefront (see include/navgpu.h)
  private_nh.param("navgpu_wavefront", wavefront, false);
  params_.tolerance_weight_dist_from_goal = 1.0;  // NavfnROS.cfg's defaults until the first reconfigure callback
  params_.tolerance_weight_path_length = 0.0;
  params_.wavefront = wavefront ? 1 : 0;

  dyncfg_srv_.reset(new dynamic_reconfigure::Server<navfn::NavfnROSConfig>(private_nh));
  dynamic_reconfigure::Server<navfn::NavfnROSConfig>::CallbackType cb = boost::bind(&NavfnROS::reconfigureCB, this, _1, _2);
  dyncfg_srv_->setCallback(cb);

  ros::NodeHandle prefix_nh;  // tf::getPrefixParam (:92-93)
  std::string key;
  if (prefix_nh.searchParam("tf_prefix", key)) prefix_nh.getParam(key, tf_prefix_);
  initialized_ = true;
}

void NavfnROS::reconfigureCB(navfn::NavfnROSConfig& config, uint32_t level) {
  (void)level;
  allow_unknown_ = config.allow_unknown;
  default_tolerance_ = config.default_tolerance;
  params_.tolerance_weight_dist_from_goal = config.tolerance_weight_dist_from_goal;
  params_.tolerance_weight_path_length = config.tolerance_weight_path_length;
}

bool NavfnROS::ensureHandle() {
  const uint32_t nx = costmap_->getSizeInCellsX(), ny = costmap_->getSizeInCellsY();
  if (handle_ && nx == nx_ && ny == ny_) return true;
  if (handle_) navgpu_navfn_destroy(handle_);
  handle_ = NULL;
  if (navgpu_navfn_create(nx, ny, 1, 0, &handle_) != NAVGPU_OK) {
    handle_ = NULL;
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  nx_ = nx;
  ny_ = ny;
  return true;
}

// planner_->setNavArr(size); planner_->setCostmap(getCharMap(), true, allow_unknown_) (:263-264, 178-179)
bool NavfnROS::loadCostmap() {
  if (!ensureHandle() || navgpu_navfn_set_costmap(handle_, 0, 1, costmap_->getCharMap(), 0, 1, allow_unknown_) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  return true;
}

void NavfnROS::frame(double out[3]) const {
  out[0] = costmap_->getOriginX();
  out[1] = costmap_->getOriginY();
  out[2] = costmap_->getResolution();
}

bool NavfnROS::validPointPotential(const geometry_msgs::Point& world_point) { return validPointPotential(world_point, default_tolerance_); }

bool NavfnROS::validPointPotential(const geometry_msgs::Point& world_point, double tolerance) {
  if (!initialized_) {
    ROS_ERROR("%s", kNotInitialized);
    return false;
  }
  if (!ensureHandle()) return false;
  double fr[3];
  frame(fr);
  const uint32_t one = 1;
  const double xy[2] = {world_point.x, world_point.y};
  int32_t flag = 0;
  if (navgpu_navfn_ros_valid_point_potential(handle_, 0, 1, fr, &one, xy, &tolerance, &flag) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  return flag != 0;
}

double NavfnROS::getPointPotential(const geometry_msgs::Point& world_point) {
  if (!initialized_) {
    ROS_ERROR("%s", kNotInitialized);
    return -1.0;
  }
  if (!ensureHandle()) return DBL_MAX;
  double fr[3];
  frame(fr);
  const uint32_t one = 1;
  const double xy[2] = {world_point.x, world_point.y};
  double potential = DBL_MAX;
  if (navgpu_navfn_ros_point_potential(handle_, 0, 1, fr, &one, xy, &potential) != NAVGPU_OK)
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
  return potential;
}

bool NavfnROS::computePotential(const geometry_msgs::Point& world_point) {
  if (!initialized_) {
    ROS_ERROR("%s", kNotInitialized);
    return false;
  }
  if (!loadCostmap()) return false;
  double fr[3];
  frame(fr);
  const double xy[2] = {world_point.x, world_point.y};
  navgpu_navfn_ros_result result;
  if (navgpu_navfn_ros_compute_potential(handle_, 0, 1, &params_, fr, xy, &result) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  return result.status == NAVGPU_MAKE_PLAN_OK && result.found;
}

bool NavfnROS::makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal,
                        std::vector<geometry_msgs::PoseStamped>& plan) {
  return makePlan(start, goal, default_tolerance_, plan);
}

bool NavfnROS::makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal, double tolerance,
                        std::vector<geometry_msgs::PoseStamped>& plan) {
  boost::unique_lock<boost::mutex> lock(mutex_);
  if (!initialized_) {
    ROS_ERROR("%s", kNotInitialized);
    return false;
  }
  plan.clear();
  const std::string global_frame = resolveFrame(tf_prefix_, global_frame_);
  if (resolveFrame(tf_prefix_, goal.header.frame_id) != global_frame) {
    ROS_ERROR("The goal pose passed to this planner must be in the %s frame.  It is instead in the %s frame.", global_frame.c_str(),
              resolveFrame(tf_prefix_, goal.header.frame_id).c_str());
    return false;
  }
  if (resolveFrame(tf_prefix_, start.header.frame_id) != global_frame) {
    ROS_ERROR("The start pose passed to this planner must be in the %s frame.  It is instead in the %s frame.", global_frame.c_str(),
              resolveFrame(tf_prefix_, start.header.frame_id).c_str());
    return false;
  }
  if (!loadCostmap()) return false;
  double fr[3];
  frame(fr);
  const double s[3] = {start.pose.position.x, start.pose.position.y, 0.0};
  const double g[3] = {goal.pose.position.x, goal.pose.position.y, 0.0};  // the goal's orientation travels with best_pose below
  navgpu_navfn_ros_result result;
  if (navgpu_navfn_ros_make_plan(handle_, 0, 1, &params_, fr, s, g, &tolerance, &result) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  if (result.status == NAVGPU_MAKE_PLAN_START_OFF_MAP) {
    ROS_WARN("The robot's start position is off the global costmap. Planning will always fail, are you sure the robot has been properly localized?");
    return false;
  }
  if (result.status == NAVGPU_MAKE_PLAN_GOAL_OFF_MAP) {
    ROS_WARN_THROTTLE(1.0, "The goal sent to the navfn planner is off the global costmap. Planning will always fail to this goal.");
    return false;
  }
  if (result.status == NAVGPU_MAKE_PLAN_NO_PLAN && result.best_cell[0] >= 0)
    ROS_ERROR("Failed to get a plan from potential when a legal potential was found. This shouldn't happen.");

  std::vector<navgpu_global_pose> poses(result.n_poses > 0 ? result.n_poses : 0);
  uint32_t offsets[2] = {0, 0};
  if (navgpu_navfn_ros_plans(handle_, 0, 1, (uint32_t)poses.size(), poses.empty() ? NULL : &poses[0], offsets) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  // getPlanFromPotential's poses (:440-456), then best_pose: a copy of the goal at the best candidate's position (:302-303, 321, 333-335)
  const ros::Time plan_time = ros::Time::now();
  for (size_t i = 0; i < poses.size(); ++i) {
    geometry_msgs::PoseStamped pose;
    if (i + 1 == poses.size()) {
      pose = goal;
      pose.header.stamp = ros::Time::now();
    } else {
      pose.header.stamp = plan_time;
      pose.header.frame_id = global_frame_;
      pose.pose.position.z = 0.0;
      pose.pose.orientation.x = 0.0;
      pose.pose.orientation.y = 0.0;
      pose.pose.orientation.z = 0.0;
      pose.pose.orientation.w = 1.0;
    }
    pose.pose.position.x = poses[i].x;
    pose.pose.position.y = poses[i].y;
    plan.push_back(pose);
  }
  if (visualize_potential_) publishPotential();
  publishPlan(plan, 0.0, 1.0, 0.0, 0.0);
  return !plan.empty();
}

void NavfnROS::publishPotential() {
  double fr[3];
  frame(fr);
  uint32_t offsets[2] = {0, 0};
  if (navgpu_navfn_ros_potential_cloud(handle_, 0, 1, fr, 0, NULL, offsets) != NAVGPU_OK) return;
  pcl::PointCloud<navgpu_navfn_ros_cloud_point> pot_area;
  pot_area.header.frame_id = global_frame_;
  pot_area.header.stamp = (uint64_t)(ros::Time::now().toSec() * 1e6);  // pcl_conversions::toPCL: microseconds
  pot_area.points.resize(offsets[1]);
  if (offsets[1] && navgpu_navfn_ros_potential_cloud(handle_, 0, 1, fr, offsets[1], &pot_area.points[0], offsets) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return;
  }
  potarr_pub_.publish(pot_area);
}

void NavfnROS::publishPlan(const std::vector<geometry_msgs::PoseStamped>& path, double r, double g, double b, double a) {
  if (!initialized_) {
    ROS_ERROR("%s", kNotInitialized);
    return;
  }
  nav_msgs::Path gui_path;
  gui_path.poses.resize(path.size());
  if (!path.empty()) {
    gui_path.header.frame_id = path[0].header.frame_id;
    gui_path.header.stamp = path[0].header.stamp;
  }
  for (unsigned int i = 0; i < path.size(); i++) gui_path.poses[i] = path[i];
  plan_pub_.publish(gui_path);
}

bool NavfnROS::getPlanFromPotential(const geometry_msgs::PoseStamped& goal, std::vector<geometry_msgs::PoseStamped>& plan) {
  if (!initialized_) {
    ROS_ERROR("%s", kNotInitialized);
    return false;
  }
  plan.clear();
  const std::string global_frame = resolveFrame(tf_prefix_, global_frame_);
  if (resolveFrame(tf_prefix_, goal.header.frame_id) != global_frame) {
    ROS_ERROR("The goal pose passed to this planner must be in the %s frame.  It is instead in the %s frame.", global_frame.c_str(),
              resolveFrame(tf_prefix_, goal.header.frame_id).c_str());
    return false;
  }
  if (!ensureHandle()) return false;
  double fr[3];
  frame(fr);
  const double g[3] = {goal.pose.position.x, goal.pose.position.y, 0.0};
  navgpu_navfn_ros_result result;
  if (navgpu_navfn_ros_plan_from_potential(handle_, 0, 1, fr, g, &result) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  if (result.status == NAVGPU_MAKE_PLAN_GOAL_OFF_MAP) {
    ROS_WARN_THROTTLE(1.0, "The goal sent to the navfn planner is off the global costmap. Planning will always fail to this goal.");
    return false;
  }
  std::vector<navgpu_global_pose> poses(result.n_poses > 0 ? result.n_poses : 0);
  uint32_t offsets[2] = {0, 0};
  if (navgpu_navfn_ros_plans(handle_, 0, 1, (uint32_t)poses.size(), poses.empty() ? NULL : &poses[0], offsets) != NAVGPU_OK) {
    ROS_ERROR("navgpu::NavfnROS: %s", navgpu_last_error());
    return false;
  }
  const ros::Time plan_time = ros::Time::now();
  for (size_t i = 0; i < poses.size(); ++i) {
    geometry_msgs::PoseStamped pose;
    pose.header.stamp = plan_time;
    pose.header.frame_id = global_frame_;
    pose.pose.position.x = poses[i].x;
    pose.pose.position.y = poses[i].y;
    pose.pose.position.z = 0.0;
    pose.pose.orientation.x = 0.0;
    pose.pose.orientation.y = 0.0;
    pose.pose.orientation.z = 0.0;
    pose.pose.orientation.w = 1.0;
    plan.push_back(pose);
  }
  publishPlan(plan, 0.0, 1.0, 0.0, 0.0);
  return !plan.empty();
}

}  // namespace navgpu
