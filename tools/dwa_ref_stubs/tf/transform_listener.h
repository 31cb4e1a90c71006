// Stand-in for <tf/transform_listener.h>, for tools/dwa_reference_harness.cpp only: the calls LocalPlannerUtil and goal_functions.cpp
// name.  The harness hands DWAPlanner plans that are already in the costmap's frame, so none of them runs; a lookup answers identity.
#pragma once
#include <tf/tf.h>
#include <sensor_msgs/PointCloud.h>
namespace tf {
class Transformer { public: virtual ~Transformer() {} };
class TransformListener : public Transformer {
 public:
  TransformListener() {}
  TransformListener(ros::Duration) {}
  void transformPose(const std::string&, const Stamped<Pose>& in, Stamped<Pose>& out) const { out = in; }
  void transformPose(const std::string&, const geometry_msgs::PoseStamped& in, geometry_msgs::PoseStamped& out) const { out = in; }
  template <class A, class B> void transformPoint(const std::string&, const A& in, B& out) const { out = in; }
  void transformPointCloud(const std::string&, const sensor_msgs::PointCloud& in, sensor_msgs::PointCloud& out) const { out = in; }
  void lookupTransform(const std::string&, const std::string&, const ros::Time&, StampedTransform& t) const { t.setIdentity(); }
  void lookupTransform(const std::string&, const ros::Time&, const std::string&, const ros::Time&, const std::string&, StampedTransform& t) const { t.setIdentity(); }
  bool waitForTransform(const std::string&, const std::string&, const ros::Time&, const ros::Duration&, const ros::Duration& = ros::Duration(), std::string* = 0) const { return true; }
  bool waitForTransform(const std::string&, const ros::Time&, const std::string&, const ros::Time&, const std::string&, const ros::Duration&, const ros::Duration& = ros::Duration(), std::string* = 0) const { return true; }
  bool canTransform(const std::string&, const std::string&, const ros::Time&, std::string* = 0) const { return true; }
  std::string resolve(const std::string& s) const { return s; }
};
}  // namespace tf
