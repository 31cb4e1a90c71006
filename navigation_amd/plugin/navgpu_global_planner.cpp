// navgpu::GlobalPlanner (navgpu_global_planner.h): global_planner::GlobalPlanner's ROS face over navgpu_global_planner_make_plan.
#include "navgpu_global_planner.h"

#include <boost/bind.hpp>
#include <costmap_2d/cost_values.h>
#include <pluginlib/class_list_macros.h>
#include <tf/tf.h>

PLUGINLIB_EXPORT_CLASS(navgpu::GlobalPlanner, nav_core::BaseGlobalPlanner)

namespace navgpu {

namespace {
// tf::resolve(prefix, frame_name) as tf documents it (tf is not part of the reference tree): an absolute name stays, a relative one
// goes under the prefix
std::string resolveFrame(const std::string& prefix, const std::string& frame_name) {
  if (!frame_name.empty() && frame_name[0] == '/') return frame_name;
  if (prefix.empty()) return "/" + frame_name;
  return (prefix[0] == '/' ? prefix : "/" + prefix) + "/" + frame_name;
}
}  // namespace

GlobalPlanner::GlobalPlanner()
    : costmap_(NULL), initialized_(false), publish_potential_(true), publish_scale_(100), planner_window_x_(0), planner_window_y_(0),
      default_tolerance_(0), params_(), options_(), handle_(NULL), nx_(0), ny_(0), dsrv_(NULL) {}

GlobalPlanner::GlobalPlanner(std::string name, costmap_2d::Costmap2D* costmap, std::string frame_id)
    : costmap_(NULL), initialized_(false), publish_potential_(true), publish_scale_(100), planner_window_x_(0), planner_window_y_(0),
      default_tolerance_(0), params_(), options_(), handle_(NULL), nx_(0), ny_(0), dsrv_(NULL) {
  initialize(name, costmap, frame_id);
}

GlobalPlanner::~GlobalPlanner() {
  if (dsrv_) delete dsrv_;
  if (handle_) navgpu_navfn_destroy(handle_);
}

void GlobalPlanner::initialize(std::string name, costmap_2d::Costmap2DROS* costmap_ros) {
  initialize(name, costmap_ros->getCostmap(), costmap_ros->getGlobalFrameID());
}

void GlobalPlanner::initialize(std::string name, costmap_2d::Costmap2D* costmap, std::string frame_id) {
  if (initialized_) {
    ROS_WARN("This planner has already been initialized, you can't call it twice, doing nothing");
    return;
  }
  ros::NodeHandle private_nh("~/" + name);
  costmap_ = costmap;
  frame_id_ = frame_id;
  bool old_navfn_behavior, use_quadratic, use_dijkstra, use_grid_path, allow_unknown;
  private_nh.param("old_navfn_behavior", old_navfn_behavior, false);
  private_nh.param("use_quadratic", use_quadratic, true);
  private_nh.param("use_dijkstra", use_dijkstra, true);
  private_nh.param("use_grid_path", use_grid_path, false);
  private_nh.param("allow_unknown", allow_unknown, true);
  private_nh.param("planner_window_x", planner_window_x_, 0.0);
  private_nh.param("planner_window_y", planner_window_y_, 0.0);
  private_nh.param("default_tolerance", default_tolerance_, 0.0);
  private_nh.param("publish_scale", publish_scale_, 100);
  bool wavefront;  // no counterpart in the reference: DijkstraExpansion as the library's tiled wavefront (see include/navgpu.h)
  private_nh.param("navgpu_wavefront", wavefront, false);
  params_.old_navfn_behavior = old_navfn_behavior;
  params_.use_quadratic = use_quadratic;
  params_.use_dijkstra = use_dijkstra;
  params_.use_grid_path = use_grid_path;
  params_.allow_unknown = allow_unknown;
  params_.lethal_cost = 253;  // GlobalPlanner.cfg's defaults until the first reconfigure callback
  params_.neutral_cost = 50;
  params_.cost_factor = 3.0f;
  params_.outline_map = 1;  // makePlan always outlines (:296)
  options_.orientation_mode = NAVGPU_ORIENT_FORWARD;
  options_.wavefront = (wavefront && use_dijkstra) ? 1 : 0;

  plan_pub_ = private_nh.advertise<nav_msgs::Path>("plan", 1);
  potential_pub_ = private_nh.advertise<nav_msgs::OccupancyGrid>("potential", 1);

  ros::NodeHandle prefix_nh;  // tf::getPrefixParam (:150-152)
  std::string key;
  if (prefix_nh.searchParam("tf_prefix", key)) prefix_nh.getParam(key, tf_prefix_);

  dsrv_ = new dynamic_reconfigure::Server<global_planner::GlobalPlannerConfig>(ros::NodeHandle("~/" + name));
  dynamic_reconfigure::Server<global_planner::GlobalPlannerConfig>::CallbackType cb = boost::bind(&GlobalPlanner::reconfigureCB, this, _1, _2);
  dsrv_->setCallback(cb);
  initialized_ = true;
}

void GlobalPlanner::reconfigureCB(global_planner::GlobalPlannerConfig& config, uint32_t level) {
  params_.lethal_cost = config.lethal_cost;
  params_.neutral_cost = config.neutral_cost;
  params_.cost_factor = (float)config.cost_factor;  // Expander::setFactor(float)
  publish_potential_ = config.publish_potential;
  options_.orientation_mode = config.orientation_mode;
}

bool GlobalPlanner::ensureHandle(uint32_t nx, uint32_t ny) {
  if (handle_ && nx == nx_ && ny == ny_) return true;
  if (handle_) navgpu_navfn_destroy(handle_);
  handle_ = NULL;
  if (navgpu_navfn_create(nx, ny, 1, 0, &handle_) != NAVGPU_OK) {
    handle_ = NULL;
    return false;
  }
  nx_ = nx;
  ny_ = ny;
  return true;
}

bool GlobalPlanner::makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal,
                             std::vector<geometry_msgs::PoseStamped>& plan) {
  return makePlan(start, goal, default_tolerance_, plan);
}

bool GlobalPlanner::makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal, double tolerance,
                             std::vector<geometry_msgs::PoseStamped>& plan) {
  boost::unique_lock<boost::mutex> lock(mutex_);
  if (!initialized_) {
    ROS_ERROR("This planner has not been initialized yet, but it is being used, please call initialize() before use");
    return false;
  }
  plan.clear();
  const std::string global_frame = resolveFrame(tf_prefix_, frame_id_);
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
  // the reference changes its own costmap before it plans (clearRobotCell, :283-286), after both worldToMap tests (:256-275)
  unsigned int start_x_i, start_y_i, goal_x_i, goal_y_i;
  if (!costmap_->worldToMap(start.pose.position.x, start.pose.position.y, start_x_i, start_y_i)) {
    ROS_WARN("The robot's start position is off the global costmap. Planning will always fail, are you sure the robot has been properly localized?");
    return false;
  }
  if (!costmap_->worldToMap(goal.pose.position.x, goal.pose.position.y, goal_x_i, goal_y_i)) {
    ROS_WARN_THROTTLE(1.0, "The goal sent to the global planner is off the global costmap. Planning will always fail to this goal.");
    return false;
  }
  costmap_->setCost(start_x_i, start_y_i, costmap_2d::FREE_SPACE);

  if (!ensureHandle(costmap_->getSizeInCellsX(), costmap_->getSizeInCellsY()) ||
      navgpu_navfn_set_costmap(handle_, 0, 1, costmap_->getCharMap(), 0, 0, params_.allow_unknown) != NAVGPU_OK) {
    ROS_ERROR("navgpu::GlobalPlanner: %s", navgpu_last_error());
    return false;
  }
  const double frame[3] = {costmap_->getOriginX(), costmap_->getOriginY(), costmap_->getResolution()};
  const double s[3] = {start.pose.position.x, start.pose.position.y, tf::getYaw(start.pose.orientation)};
  const double g[3] = {goal.pose.position.x, goal.pose.position.y, tf::getYaw(goal.pose.orientation)};
  navgpu_make_plan_result result;
  if (navgpu_global_planner_make_plan(handle_, 0, 1, &params_, &options_, frame, s, g, &result) != NAVGPU_OK) {
    ROS_ERROR("navgpu::GlobalPlanner: %s", navgpu_last_error());
    return false;
  }
  if (publish_potential_) publishPotential();  // :303-304
  if (result.status == NAVGPU_MAKE_PLAN_BORDER)
    ROS_ERROR("navgpu::GlobalPlanner: start closer than 2 cells or goal closer than 1 cell to the costmap's border");
  else if (result.status != NAVGPU_MAKE_PLAN_OK)
    ROS_ERROR("Failed to get a plan.");

  std::vector<navgpu_global_pose> poses(result.n_poses > 0 ? result.n_poses : 0);
  uint32_t offsets[2] = {0, 0};
  if (navgpu_global_planner_plans(handle_, 0, 1, (uint32_t)poses.size(), poses.empty() ? NULL : &poses[0], offsets) != NAVGPU_OK) {
    ROS_ERROR("navgpu::GlobalPlanner: %s", navgpu_last_error());
    return false;
  }
  // getPlanFromPotential's poses (:372-393), the goal (with old_navfn_behavior) and goal_copy (:310-312); an orientation is written
  // wherever processPath writes one: nowhere with NONE, everywhere but the last pose with FORWARD, everywhere otherwise
  const ros::Time plan_time = ros::Time::now();
  const size_t n = poses.size(), n_goal = params_.old_navfn_behavior ? 2 : 1;
  for (size_t i = 0; i < n; ++i) {
    geometry_msgs::PoseStamped pose;
    if (i + n_goal >= n) {
      pose = goal;
      if (i + 1 == n) pose.header.stamp = ros::Time::now();
    } else {
      pose.header.stamp = plan_time;
      pose.header.frame_id = frame_id_;
      pose.pose.position.x = poses[i].x;
      pose.pose.position.y = poses[i].y;
      pose.pose.position.z = 0.0;
      pose.pose.orientation.x = 0.0;
      pose.pose.orientation.y = 0.0;
      pose.pose.orientation.z = 0.0;
      pose.pose.orientation.w = 1.0;
    }
    const bool written = options_.orientation_mode != NAVGPU_ORIENT_NONE && !(options_.orientation_mode == NAVGPU_ORIENT_FORWARD && i + 1 == n);
    if (written) pose.pose.orientation = tf::createQuaternionMsgFromYaw(poses[i].yaw);
    plan.push_back(pose);
  }
  publishPlan(plan);
  return !plan.empty();
}

void GlobalPlanner::publishPlan(const std::vector<geometry_msgs::PoseStamped>& path) {
  if (!initialized_) {
    ROS_ERROR("This planner has not been initialized yet, but it is being used, please call initialize() before use");
    return;
  }
  nav_msgs::Path gui_path;
  gui_path.poses.resize(path.size());
  gui_path.header.frame_id = frame_id_;
  gui_path.header.stamp = ros::Time::now();
  for (unsigned int i = 0; i < path.size(); i++) gui_path.poses[i] = path[i];
  plan_pub_.publish(gui_path);
}

void GlobalPlanner::publishPotential() {
  const double resolution = costmap_->getResolution();
  nav_msgs::OccupancyGrid grid;
  grid.header.frame_id = frame_id_;
  grid.header.stamp = ros::Time::now();
  grid.info.resolution = resolution;
  grid.info.width = nx_;
  grid.info.height = ny_;
  double wx, wy;
  costmap_->mapToWorld(0, 0, wx, wy);
  grid.info.origin.position.x = wx - resolution / 2;
  grid.info.origin.position.y = wy - resolution / 2;
  grid.info.origin.position.z = 0.0;
  grid.info.origin.orientation.w = 1.0;
  grid.data.resize((size_t)nx_ * ny_);
  if (navgpu_global_planner_potential_grid(handle_, 0, 1, publish_scale_, &grid.data[0], NULL) != NAVGPU_OK) {
    ROS_ERROR("navgpu::GlobalPlanner: %s", navgpu_last_error());
    return;
  }
  potential_pub_.publish(grid);
}

}  // namespace navgpu
