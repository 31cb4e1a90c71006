// navgpu::GlobalPlanner - stand-in for global_planner::GlobalPlanner (global_planner/include/global_planner/planner_core.h:61-196) over
// the navgpu C-ABI: one makePlan is
//   navgpu_navfn_set_costmap (getCharMap(), cost_mode 0) -> navgpu_global_planner_make_plan -> navgpu_global_planner_plans
//   (-> navgpu_global_planner_potential_grid when publish_potential)
// on a navgpu_navfn handle of one plan.  Expansion, traceback, plan assembly and the orientation filter run on the device; this class
// keeps the reference's parameters, frame checks, warnings and publishers.  Not offered: the make_plan service (planner_core.cpp:154,
// 187-194) and getPlanFromPotential / computePotential as separate public calls.  An executive that plans for many robots calls the
// C-ABI with a range of plans instead.  Source-only in this repository (needs the ROS headers).
#ifndef NAVGPU_GLOBAL_PLANNER_H_
#define NAVGPU_GLOBAL_PLANNER_H_
#include <string>
#include <vector>

#include <boost/thread/mutex.hpp>
#include <costmap_2d/costmap_2d.h>
#include <costmap_2d/costmap_2d_ros.h>
#include <dynamic_reconfigure/server.h>
#include <geometry_msgs/PoseStamped.h>
#include <global_planner/GlobalPlannerConfig.h>
#include <nav_core/base_global_planner.h>
#include <nav_msgs/OccupancyGrid.h>
#include <nav_msgs/Path.h>
#include <ros/ros.h>

#include "navgpu.h"

namespace navgpu {

class GlobalPlanner : public nav_core::BaseGlobalPlanner {
 public:
  GlobalPlanner();
  GlobalPlanner(std::string name, costmap_2d::Costmap2D* costmap, std::string frame_id);
  ~GlobalPlanner();
  void initialize(std::string name, costmap_2d::Costmap2DROS* costmap_ros);                  // planner_core.cpp:91-93
  void initialize(std::string name, costmap_2d::Costmap2D* costmap, std::string frame_id);  // :95-165
  using nav_core::BaseGlobalPlanner::makePlan;                                               // (the overload with a cost)
  bool makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal,
                std::vector<geometry_msgs::PoseStamped>& plan);                              // :217-220
  bool makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal, double tolerance,
                std::vector<geometry_msgs::PoseStamped>& plan);                              // :222-327
  void publishPlan(const std::vector<geometry_msgs::PoseStamped>& path);                     // :329-349

 private:
  void reconfigureCB(global_planner::GlobalPlannerConfig& config, uint32_t level);           // :167-174
  bool ensureHandle(uint32_t nx, uint32_t ny);
  void publishPotential();                                                                   // :397-436

  costmap_2d::Costmap2D* costmap_;
  std::string frame_id_, tf_prefix_;
  ros::Publisher plan_pub_, potential_pub_;
  bool initialized_, publish_potential_;
  int publish_scale_;
  double planner_window_x_, planner_window_y_, default_tolerance_;  // read as the reference reads them; it never uses them either
  navgpu_global_planner_params params_;
  navgpu_make_plan_options options_;
  navgpu_navfn* handle_;
  uint32_t nx_, ny_;
  boost::mutex mutex_;
  dynamic_reconfigure::Server<global_planner::GlobalPlannerConfig>* dsrv_;
};

}  // namespace navgpu
#endif
