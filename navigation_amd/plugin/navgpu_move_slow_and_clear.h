// navgpu::MoveSlowAndClear - a stand-in for move_slow_and_clear::MoveSlowAndClear
// (move_slow_and_clear/include/move_slow_and_clear/move_slow_and_clear.h:48-85) whose clearing reaches obstacle layers that live on
// the device:
//   MoveSlowAndClear::runBehavior's setConvexPolygonCost on every "obstacles" layer (move_slow_and_clear.cpp:83-127)
//                                             -> navgpu_costmap_set_polygon_cost(NAVGPU_GRID_OBSTACLE) for a navgpu::ObstacleLayer
//                                                (navgpu::VoxelLayer and navgpu::GpuLayers are ones), the reference's call for any other
// The speed limit stays what it is in the reference, two dynamic_reconfigure calls on the local planner and a timer that lifts it
// (:129-153, 168-223).  An executive whose costmaps already live in a fleet calls navgpu_costmap_set_polygon_cost on that fleet for
// all its robots at once.  Source-only in this repository (needs the ROS headers).
#ifndef NAVGPU_MOVE_SLOW_AND_CLEAR_H_
#define NAVGPU_MOVE_SLOW_AND_CLEAR_H_

#include <costmap_2d/costmap_2d_ros.h>
#include <nav_core/recovery_behavior.h>
#include <ros/ros.h>
#include <ros/service.h>
#include <tf/transform_listener.h>

#include <boost/thread.hpp>

#include <navgpu.h>

#include <string>
#include <vector>

namespace navgpu {

class MoveSlowAndClear : public nav_core::RecoveryBehavior {
 public:
  MoveSlowAndClear();
  ~MoveSlowAndClear();
  void initialize(std::string name, tf::TransformListener* tf, costmap_2d::Costmap2DROS* global_costmap,
                  costmap_2d::Costmap2DROS* local_costmap);  // move_slow_and_clear.cpp:54-72
  void runBehavior();                                        // :74-153

 private:
  // the square of half side clearing_distance_ round a costmap's robot pose, in the reference's vertex order (:89-106)
  static std::vector<geometry_msgs::Point> clearingPolygon(const tf::Stamped<tf::Pose>& pose, double clearing_distance);
  // FREE_SPACE inside the polygon in every layer of the costmap whose name contains "obstacles" (:109-127)
  static void clearObstacleLayers(costmap_2d::Costmap2DROS* costmap, const std::vector<geometry_msgs::Point>& polygon);
  void setRobotSpeed(double trans_speed, double rot_speed);  // :192-223
  void distanceCheck(const ros::TimerEvent& e);              // :168-183
  void removeSpeedLimit();                                   // :185-190
  double sqDistanceMoved();                                  // :155-166

  ros::NodeHandle private_nh_;
  costmap_2d::Costmap2DROS *global_costmap_, *local_costmap_;
  bool initialized_;
  double clearing_distance_, limited_trans_speed_, limited_rot_speed_, limited_distance_, old_trans_speed_, old_rot_speed_;
  std::string planner_namespace_;
  ros::Timer distance_check_timer_;
  tf::Stamped<tf::Pose> speed_limit_pose_;
  boost::thread* remove_limit_thread_;
  boost::mutex mutex_;
  bool limit_set_;
  ros::ServiceClient planner_reconfigure_;
};

}  // namespace navgpu
#endif
