// See navgpu_move_slow_and_clear.h.  Comments cite the reference lines each block stands in for.
#include "navgpu_move_slow_and_clear.h"

#include "navgpu_layers.h"

#include <costmap_2d/obstacle_layer.h>
#include <dynamic_reconfigure/Reconfigure.h>
#include <pluginlib/class_list_macros.h>

PLUGINLIB_EXPORT_CLASS(navgpu::MoveSlowAndClear, nav_core::RecoveryBehavior)

namespace navgpu {

MoveSlowAndClear::MoveSlowAndClear()
    : global_costmap_(NULL), local_costmap_(NULL), initialized_(false), clearing_distance_(0.5), limited_trans_speed_(0.25),
      limited_rot_speed_(0.45), limited_distance_(0.3), old_trans_speed_(0.0), old_rot_speed_(0.0), remove_limit_thread_(NULL),
      limit_set_(false) {}

MoveSlowAndClear::~MoveSlowAndClear() {
  if (remove_limit_thread_) {
    remove_limit_thread_->join();
    delete remove_limit_thread_;
  }
}

void MoveSlowAndClear::initialize(std::string name, tf::TransformListener* tf, costmap_2d::Costmap2DROS* global_costmap,
                                  costmap_2d::Costmap2DROS* local_costmap) {
  global_costmap_ = global_costmap;
  local_costmap_ = local_costmap;
  private_nh_ = ros::NodeHandle("~/" + name);
  private_nh_.param("clearing_distance", clearing_distance_, 0.5);  // :62-65
  private_nh_.param("limited_trans_speed", limited_trans_speed_, 0.25);
  private_nh_.param("limited_rot_speed", limited_rot_speed_, 0.45);
  private_nh_.param("limited_distance", limited_distance_, 0.3);
  private_nh_.param("planner_namespace", planner_namespace_, std::string("DWAPlannerROS"));  // :67-70
  planner_reconfigure_ = ros::service::createClient<dynamic_reconfigure::Reconfigure>("~/" + planner_namespace_ + "/set_parameters", true);
  initialized_ = true;
}

std::vector<geometry_msgs::Point> MoveSlowAndClear::clearingPolygon(const tf::Stamped<tf::Pose>& pose, double clearing_distance) {
  std::vector<geometry_msgs::Point> polygon;
  for (int i = -1; i <= 1; i += 2) {
    geometry_msgs::Point pt;
    pt.x = pose.getOrigin().x() + i * clearing_distance;
    pt.y = pose.getOrigin().y() + i * clearing_distance;
    polygon.push_back(pt);
    pt.x = pose.getOrigin().x() + i * clearing_distance;
    pt.y = pose.getOrigin().y() + -1.0 * i * clearing_distance;
    polygon.push_back(pt);
  }
  return polygon;
}

void MoveSlowAndClear::clearObstacleLayers(costmap_2d::Costmap2DROS* costmap, const std::vector<geometry_msgs::Point>& polygon) {
  std::vector<boost::shared_ptr<costmap_2d::Layer> >* plugins = costmap->getLayeredCostmap()->getPlugins();
  for (size_t k = 0; k < plugins->size(); ++k) {
    costmap_2d::Layer* layer = (*plugins)[k].get();
    if (layer->getName().find("obstacles") == std::string::npos) continue;
    if (ObstacleLayer* on_device = dynamic_cast<ObstacleLayer*>(layer)) {
      if (!on_device->setConvexPolygonCostOnDevice(polygon, costmap_2d::FREE_SPACE))
        ROS_ERROR("Move slow and clear: %s", navgpu_last_error());
    } else {  // a layer whose grid lives on the host: the reference's own call (:113-115)
      static_cast<costmap_2d::ObstacleLayer*>(layer)->setConvexPolygonCost(polygon, costmap_2d::FREE_SPACE);
    }
  }
}

void MoveSlowAndClear::runBehavior() {
  if (!initialized_) {
    ROS_ERROR("This recovery behavior has not been initialized, doing nothing.");
    return;
  }
  ROS_WARN("Move slow and clear recovery behavior started.");
  tf::Stamped<tf::Pose> global_pose, local_pose;
  global_costmap_->getRobotPose(global_pose);
  local_costmap_->getRobotPose(local_pose);
  clearObstacleLayers(global_costmap_, clearingPolygon(global_pose, clearing_distance_));
  clearObstacleLayers(local_costmap_, clearingPolygon(local_pose, clearing_distance_));

  boost::unique_lock<boost::mutex> l(mutex_);  // :129-152
  if (!limit_set_) {
    ros::NodeHandle planner_nh("~/" + planner_namespace_);
    if (!planner_nh.getParam("max_trans_vel", old_trans_speed_))
      ROS_ERROR("The planner %s, does not have the parameter max_trans_vel", planner_nh.getNamespace().c_str());
    if (!planner_nh.getParam("max_rot_vel", old_rot_speed_))
      ROS_ERROR("The planner %s, does not have the parameter max_rot_vel", planner_nh.getNamespace().c_str());
  }
  speed_limit_pose_ = global_pose;
  setRobotSpeed(limited_trans_speed_, limited_rot_speed_);
  limit_set_ = true;
  distance_check_timer_ = private_nh_.createTimer(ros::Duration(0.1), &MoveSlowAndClear::distanceCheck, this);
}

double MoveSlowAndClear::sqDistanceMoved() {
  tf::Stamped<tf::Pose> global_pose;
  global_costmap_->getRobotPose(global_pose);
  const double dx = speed_limit_pose_.getOrigin().x() - global_pose.getOrigin().x();
  const double dy = speed_limit_pose_.getOrigin().y() - global_pose.getOrigin().y();
  return dx * dx + dy * dy;
}

void MoveSlowAndClear::distanceCheck(const ros::TimerEvent& e) {
  if (limited_distance_ * limited_distance_ > sqDistanceMoved()) return;
  ROS_INFO("Moved far enough, removing speed limit.");
  if (remove_limit_thread_) {  // (a service call from a timer callback is made from a thread of its own, as in the reference)
    remove_limit_thread_->join();
    delete remove_limit_thread_;
  }
  remove_limit_thread_ = new boost::thread(boost::bind(&MoveSlowAndClear::removeSpeedLimit, this));
  distance_check_timer_.stop();
}

void MoveSlowAndClear::removeSpeedLimit() {
  boost::unique_lock<boost::mutex> l(mutex_);
  setRobotSpeed(old_trans_speed_, old_rot_speed_);
  limit_set_ = false;
}

void MoveSlowAndClear::setRobotSpeed(double trans_speed, double rot_speed) {
  const char* names[2] = {"max_trans_vel", "max_rot_vel"};
  const double values[2] = {trans_speed, rot_speed};
  for (int k = 0; k < 2; ++k) {  // one call per parameter, as the reference makes them
    dynamic_reconfigure::Reconfigure reconfigure;
    dynamic_reconfigure::DoubleParameter p;
    p.name = names[k];
    p.value = values[k];
    reconfigure.request.config.doubles.push_back(p);
    try {
      planner_reconfigure_.call(reconfigure);
      ROS_INFO("Recovery setting %s: %f", names[k], values[k]);
    } catch (...) {
      ROS_ERROR("Something went wrong in the service call to dynamic_reconfigure");
    }
  }
}

}  // namespace navgpu
