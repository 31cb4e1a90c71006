// See navgpu_recovery_plugins.h.  Comments cite the reference lines each block stands in for.
#include "navgpu_recovery_plugins.h"

#include <geometry_msgs/Twist.h>
#include <pluginlib/class_list_macros.h>

PLUGINLIB_EXPORT_CLASS(navgpu::RotateRecovery, nav_core::RecoveryBehavior)
PLUGINLIB_EXPORT_CLASS(navgpu::CarrotPlanner, nav_core::BaseGlobalPlanner)

namespace navgpu {

CostmapMirror::~CostmapMirror() {
  if (fleet_) navgpu_fleet_destroy(fleet_);
}

bool CostmapMirror::refresh(costmap_2d::Costmap2DROS* costmap_ros) {
  costmap_2d::Costmap2D* costmap = costmap_ros->getCostmap();
  boost::unique_lock<costmap_2d::Costmap2D::mutex_t> lock(*(costmap->getMutex()));
  if (!fleet_ || costmap->getSizeInCellsX() != size_x_ || costmap->getSizeInCellsY() != size_y_ || costmap->getResolution() != resolution_) {
    if (fleet_) navgpu_fleet_destroy(fleet_);
    fleet_ = NULL;
    navgpu_fleet_desc d = {};
    d.n_instances = 1;
    d.size_x = size_x_ = costmap->getSizeInCellsX();
    d.size_y = size_y_ = costmap->getSizeInCellsY();
    d.resolution = resolution_ = costmap->getResolution();
    d.layers = NAVGPU_LAYER_OBSTACLE;  // queries only: the master grid is uploaded before each of them
    d.max_footprint = 32;
    if (navgpu_fleet_create(&d, &fleet_) != NAVGPU_OK) {
      fleet_ = NULL;
      return false;
    }
    ++generation_;
  }
  std::vector<geometry_msgs::Point> footprint = costmap_ros->getRobotFootprint();
  std::vector<double> xy;
  for (size_t i = 0; i < footprint.size(); ++i) {
    xy.push_back(footprint[i].x);
    xy.push_back(footprint[i].y);
  }
  double origin[2] = {costmap->getOriginX(), costmap->getOriginY()};
  return navgpu_set_footprint(fleet_, 0, 1, xy.empty() ? NULL : &xy[0], (uint32_t)footprint.size()) == NAVGPU_OK &&
         navgpu_fleet_set_origin(fleet_, 0, 1, origin) == NAVGPU_OK &&
         navgpu_grid_upload(fleet_, NAVGPU_GRID_MASTER, 0, 1, costmap->getCharMap()) == NAVGPU_OK;
}

RotateRecovery::RotateRecovery() : global_costmap_(NULL), local_costmap_(NULL), tf_(NULL), initialized_(false), frequency_(20.0), configured_generation_(0) {}

void RotateRecovery::initialize(std::string name, tf::TransformListener* tf, costmap_2d::Costmap2DROS* global_costmap,
                                costmap_2d::Costmap2DROS* local_costmap) {
  if (initialized_) {
    ROS_ERROR("You should not call initialize twice on this object, doing nothing");
    return;
  }
  name_ = name;
  tf_ = tf;
  global_costmap_ = global_costmap;
  local_costmap_ = local_costmap;
  ros::NodeHandle private_nh("~/" + name_);
  ros::NodeHandle blp_nh("~/TrajectoryPlannerROS");
  navgpu_rotate_recovery_params p = {};
  private_nh.param("sim_granularity", p.sim_granularity, 0.017);  // :60-66
  private_nh.param("frequency", frequency_, 20.0);
  blp_nh.param("acc_lim_th", p.acc_lim_th, 3.2);
  blp_nh.param("max_rotational_vel", p.max_rotational_vel, 1.0);
  blp_nh.param("min_in_place_rotational_vel", p.min_in_place_rotational_vel, 0.4);
  blp_nh.param("yaw_goal_tolerance", p.yaw_goal_tolerance, 0.10);
  // CostmapModel(*local_costmap_->getCostmap()) (:68): allow_unknown_ from the costmap's default value (costmap_model.cpp:45-48)
  p.allow_unknown = costmap_2d::Costmap2D(*local_costmap_->getCostmap()).getDefaultValue() == 0 ? 0 : 1;
  params_ = p;
  initialized_ = true;
}

void RotateRecovery::runBehavior() {
  if (!initialized_) {
    ROS_ERROR("This object must be initialized before runBehavior is called");
    return;
  }
  if (global_costmap_ == NULL || local_costmap_ == NULL) {
    ROS_ERROR("The costmaps passed to the RotateRecovery object cannot be NULL. Doing nothing.");
    return;
  }
  ROS_WARN("Rotate recovery behavior started.");
  ros::Rate r(frequency_);
  ros::NodeHandle n;
  ros::Publisher vel_pub = n.advertise<geometry_msgs::Twist>("cmd_vel", 10);
  tf::Stamped<tf::Pose> global_pose;
  navgpu_rotate_recovery_state state = {};  // started = 0: the first step takes start_offset from the pose (:100-104)
  while (n.ok()) {
    local_costmap_->getRobotPose(global_pose);
    bool ok = mirror_.refresh(local_costmap_);
    if (ok && configured_generation_ != mirror_.generation()) {  // a fresh fleet (first tick, or the costmap was resized)
      ok = navgpu_rotate_recovery_configure(mirror_.fleet(), &params_) == NAVGPU_OK;
      if (ok) configured_generation_ = mirror_.generation();
    }
    if (!ok) {
      ROS_ERROR("Rotate recovery: %s", navgpu_last_error());
      return;
    }
    const double pose[3] = {global_pose.getOrigin().x(), global_pose.getOrigin().y(), tf::getYaw(global_pose.getRotation())};
    double cmd_wz = 0.0;
    int32_t status = NAVGPU_ROTATE_BLOCKED;
    if (navgpu_rotate_recovery_step(mirror_.fleet(), 0, 1, pose, &state, &cmd_wz, &status) != NAVGPU_OK) {
      ROS_ERROR("Rotate recovery: %s", navgpu_last_error());
      return;
    }
    if (status == NAVGPU_ROTATE_BLOCKED) {  // :123-126
      ROS_ERROR("Rotate recovery can't rotate in place because there is a potential collision. Cost: %.2f", -1.0);
      return;
    }
    geometry_msgs::Twist cmd_vel;  // :137-142
    cmd_vel.linear.x = 0.0;
    cmd_vel.linear.y = 0.0;
    cmd_vel.angular.z = cmd_wz;
    vel_pub.publish(cmd_vel);
    if (status == NAVGPU_ROTATE_DONE) return;  // :148-150
    r.sleep();
  }
}

CarrotPlanner::CarrotPlanner() : costmap_ros_(NULL), initialized_(false), allow_unknown_(0) {}

CarrotPlanner::CarrotPlanner(std::string name, costmap_2d::Costmap2DROS* costmap_ros) : costmap_ros_(NULL), initialized_(false), allow_unknown_(0) {
  initialize(name, costmap_ros);
}

void CarrotPlanner::initialize(std::string name, costmap_2d::Costmap2DROS* costmap_ros) {
  if (initialized_) {
    ROS_WARN("This planner has already been initialized... doing nothing");
    return;
  }
  costmap_ros_ = costmap_ros;
  // CostmapModel(*costmap_) (:61): allow_unknown_ from the costmap's default value (costmap_model.cpp:45-48).  step_size and
  // min_dist_from_robot (:59-60) are read by the reference and never used.
  allow_unknown_ = costmap_2d::Costmap2D(*costmap_ros_->getCostmap()).getDefaultValue() == 0 ? 0 : 1;
  initialized_ = true;
}

bool CarrotPlanner::makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal,
                             std::vector<geometry_msgs::PoseStamped>& plan) {
  if (!initialized_) {
    ROS_ERROR("The planner has not been initialized, please call initialize() to use the planner");
    return false;
  }
  plan.clear();
  if (goal.header.frame_id != costmap_ros_->getGlobalFrameID()) {  // :100-104
    ROS_ERROR("This planner as configured will only accept goals in the %s frame, but a goal was sent in the %s frame.",
              costmap_ros_->getGlobalFrameID().c_str(), goal.header.frame_id.c_str());
    return false;
  }
  tf::Stamped<tf::Pose> goal_tf, start_tf;  // :106-114
  poseStampedMsgToTF(goal, goal_tf);
  poseStampedMsgToTF(start, start_tf);
  double useless_pitch, useless_roll, goal_yaw, start_yaw;
  start_tf.getBasis().getEulerYPR(start_yaw, useless_pitch, useless_roll);
  goal_tf.getBasis().getEulerYPR(goal_yaw, useless_pitch, useless_roll);
  const double s[3] = {start.pose.position.x, start.pose.position.y, start_yaw};
  const double g[3] = {goal.pose.position.x, goal.pose.position.y, goal_yaw};
  double target[3] = {s[0], s[1], s[2]};
  int32_t found = 0;
  if (!mirror_.refresh(costmap_ros_) || navgpu_carrot_plan(mirror_.fleet(), 0, 1, s, g, allow_unknown_, target, &found) != NAVGPU_OK) {
    ROS_ERROR("Carrot planner: %s", navgpu_last_error());
    return false;
  }
  if (!found) ROS_WARN("The carrot planner could not find a valid plan for this goal");  // :141
  plan.push_back(start);  // :156-169
  geometry_msgs::PoseStamped new_goal = goal;
  new_goal.pose.position.x = target[0];
  new_goal.pose.position.y = target[1];
  new_goal.pose.orientation = tf::createQuaternionMsgFromYaw(target[2]);
  plan.push_back(new_goal);
  return found != 0;
}

}  // namespace navgpu
