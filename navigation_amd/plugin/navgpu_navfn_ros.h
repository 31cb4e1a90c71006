// navgpu::NavfnROS - stand-in for navfn::NavfnROS (navfn/include/navfn/navfn_ros.h:60-199) over the navgpu C-ABI: one makePlan is
//   navgpu_navfn_set_costmap (getCharMap(), cost_mode 1) -> navgpu_navfn_ros_make_plan -> navgpu_navfn_ros_plans
//   (-> navgpu_navfn_ros_potential_cloud when visualize_potential and somebody listens)
// on a navgpu_navfn handle of one plan.  The expansion, the tolerance search, the second calcPath, the plan assembly and the
// potential queries run on the device; this class keeps the reference's parameters, frame checks, warnings and publishers.
// Not offered: the make_plan service (navfn_ros.cpp:95, 199-206) and the private-costmap option of initialize (:116-122).  An
// executive that plans for many robots calls the C-ABI with a range of plans instead.  Source-only in this repository (needs the
// ROS headers).
#ifndef NAVGPU_NAVFN_ROS_H_
#define NAVGPU_NAVFN_ROS_H_
#include <string>
#include <vector>

#include <boost/shared_ptr.hpp>
#include <boost/thread/mutex.hpp>
#include <costmap_2d/costmap_2d.h>
#include <costmap_2d/costmap_2d_ros.h>
#include <dynamic_reconfigure/server.h>
#include <geometry_msgs/Point.h>
#include <geometry_msgs/PoseStamped.h>
#include <nav_core/base_global_planner.h>
#include <nav_msgs/Path.h>
#include <navfn/NavfnROSConfig.h>
#include <pcl_ros/publisher.h>
#include <ros/ros.h>

#include "navgpu.h"

namespace navgpu {

class NavfnROS : public nav_core::BaseGlobalPlanner {
 public:
  NavfnROS();
  NavfnROS(std::string name, costmap_2d::Costmap2DROS* costmap_ros);
  NavfnROS(std::string name, costmap_2d::Costmap2D* costmap, std::string global_frame);
  ~NavfnROS();
  void initialize(std::string name, costmap_2d::Costmap2DROS* costmap_ros);                      // navfn_ros.cpp:114-124
  void initialize(std::string name, costmap_2d::Costmap2D* costmap, std::string global_frame);  // :67-101
  using nav_core::BaseGlobalPlanner::makePlan;                                                   // (the overload with a cost)
  bool makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal,
                std::vector<geometry_msgs::PoseStamped>& plan);                                  // :213-216
  bool makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal, double tolerance,
                std::vector<geometry_msgs::PoseStamped>& plan);                                  // :218-374
  bool computePotential(const geometry_msgs::Point& world_point);                                // :171-197
  bool getPlanFromPotential(const geometry_msgs::PoseStamped& goal, std::vector<geometry_msgs::PoseStamped>& plan);  // :400-461
  double getPointPotential(const geometry_msgs::Point& world_point);                             // :157-169
  bool validPointPotential(const geometry_msgs::Point& world_point);                             // :126-128
  bool validPointPotential(const geometry_msgs::Point& world_point, double tolerance);           // :130-155
  void publishPlan(const std::vector<geometry_msgs::PoseStamped>& path, double r, double g, double b, double a);  // :376-398

 private:
  void reconfigureCB(navfn::NavfnROSConfig& config, uint32_t level);                             // :103-112
  bool ensureHandle();
  bool loadCostmap();
  void frame(double out[3]) const;
  void publishPotential();                                                                       // :342-368

  costmap_2d::Costmap2D* costmap_;
  std::string global_frame_, tf_prefix_;
  ros::Publisher plan_pub_;
  pcl_ros::Publisher<navgpu_navfn_ros_cloud_point> potarr_pub_;
  bool initialized_, allow_unknown_, visualize_potential_;
  double planner_window_x_, planner_window_y_, default_tolerance_;  // the windows are read as the reference reads them; it never uses them either
  navgpu_navfn_ros_params params_;
  navgpu_navfn* handle_;
  uint32_t nx_, ny_;
  boost::mutex mutex_;
  boost::shared_ptr<dynamic_reconfigure::Server<navfn::NavfnROSConfig> > dyncfg_srv_;
};

}  // namespace navgpu
#endif
