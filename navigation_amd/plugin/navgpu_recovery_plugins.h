// navgpu::RotateRecovery and navgpu::CarrotPlanner - stand-ins for rotate_recovery::RotateRecovery
// (rotate_recovery/include/rotate_recovery/rotate_recovery.h:50-83) and carrot_planner::CarrotPlanner
// (carrot_planner/include/carrot_planner/carrot_planner.h:58-104) over the navgpu C-ABI.  Both are loops around
// CostmapModel::footprintCost; here each loop pass (RotateRecovery) or the whole search (CarrotPlanner) is one call:
//   RotateRecovery::runBehavior, per tick   -> navgpu_rotate_recovery_step
//   CarrotPlanner::makePlan                 -> navgpu_carrot_plan
// Each object keeps a fleet of one robot and hands it the borrowed costmap's bytes and origin before it asks (as
// navgpu::TrajectoryPlanner does); an executive whose costmaps already live in a fleet calls the C-ABI on that fleet directly
// and nothing crosses PCIe.  Source-only in this repository (needs the ROS headers).
#ifndef NAVGPU_RECOVERY_PLUGINS_H_
#define NAVGPU_RECOVERY_PLUGINS_H_

#include <costmap_2d/costmap_2d_ros.h>
#include <geometry_msgs/PoseStamped.h>
#include <nav_core/base_global_planner.h>
#include <nav_core/recovery_behavior.h>
#include <ros/ros.h>
#include <tf/transform_listener.h>

#include <navgpu.h>

#include <string>
#include <vector>

namespace navgpu {

// one robot's costmap on the device: created for the costmap's size, refreshed (bytes, origin, footprint) before a query
class CostmapMirror {
 public:
  CostmapMirror() : fleet_(NULL), generation_(0), size_x_(0), size_y_(0), resolution_(0.0) {}
  ~CostmapMirror();
  // false when the device refuses (navgpu_last_error says why)
  bool refresh(costmap_2d::Costmap2DROS* costmap_ros);
  navgpu_fleet* fleet() { return fleet_; }
  unsigned int generation() const { return generation_; }  // bumped whenever the fleet is created anew: its configuration starts over

 private:
  CostmapMirror(const CostmapMirror&);
  CostmapMirror& operator=(const CostmapMirror&);
  navgpu_fleet* fleet_;
  unsigned int generation_;
  unsigned int size_x_, size_y_;
  double resolution_;
};

class RotateRecovery : public nav_core::RecoveryBehavior {
 public:
  RotateRecovery();
  void initialize(std::string name, tf::TransformListener* tf, costmap_2d::Costmap2DROS* global_costmap,
                  costmap_2d::Costmap2DROS* local_costmap);  // rotate_recovery.cpp:47-75
  void runBehavior();                                        // :81-154

 private:
  costmap_2d::Costmap2DROS *global_costmap_, *local_costmap_;
  tf::TransformListener* tf_;
  bool initialized_;
  std::string name_;
  double frequency_;
  navgpu_rotate_recovery_params params_;
  CostmapMirror mirror_;
  unsigned int configured_generation_;  // mirror_.generation() the parameters were last handed to
};

class CarrotPlanner : public nav_core::BaseGlobalPlanner {
 public:
  CarrotPlanner();
  CarrotPlanner(std::string name, costmap_2d::Costmap2DROS* costmap_ros);
  void initialize(std::string name, costmap_2d::Costmap2DROS* costmap_ros);  // carrot_planner.cpp:53-67
  using nav_core::BaseGlobalPlanner::makePlan;                               // (the overload with a cost)
  bool makePlan(const geometry_msgs::PoseStamped& start, const geometry_msgs::PoseStamped& goal,
                std::vector<geometry_msgs::PoseStamped>& plan);              // :87-170

 private:
  costmap_2d::Costmap2DROS* costmap_ros_;
  bool initialized_;
  int allow_unknown_;
  CostmapMirror mirror_;
};

}  // namespace navgpu
#endif
