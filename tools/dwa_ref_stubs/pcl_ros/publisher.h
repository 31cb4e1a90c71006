// Stand-in for <pcl_ros/publisher.h>, for tools/dwa_reference_harness.cpp only: a publisher of point clouds that sends nothing.
#pragma once
#include <ros/ros.h>
#include <pcl/point_cloud.h>
#include <pcl_conversions/pcl_conversions.h>
namespace pcl_ros {
template <class T> class Publisher {
 public:
  void advertise(ros::NodeHandle&, const std::string&, uint32_t) {}
  template <class C> void publish(const C&) const {}
};
}  // namespace pcl_ros
