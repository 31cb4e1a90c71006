// Stand-in for <pcl_ros/transforms.h> and the two PCL headers observation_buffer.cpp names beside it, for
// tools/costmap_reference_harness.cpp only, written from the packages' documentation.  ObstacleLayer creates an ObservationBuffer per
// observation source; the harness configures no source and hands the layer its observations through addStaticObservation, so nothing
// declared here runs: it lets observation_buffer.cpp compile and link.  A transform into another frame copies (the identity).
#pragma once
#include <stdexcept>
#include <string>
#include <pcl/point_cloud.h>
#include <pcl_conversions/pcl_conversions.h>
#include <sensor_msgs/PointCloud2.h>
#include <tf/transform_listener.h>
#include <geometry_msgs/Point.h>
#include <std_msgs/Header.h>
namespace geometry_msgs {
struct PointStamped { std_msgs::Header header; Point point; };
}  // namespace geometry_msgs
namespace ros {
inline bool operator==(const Duration& a, const Duration& b) { return a.toSec() == b.toSec(); }
inline bool operator>(const Duration& a, const Duration& b) { return a.toSec() > b.toSec(); }
}  // namespace ros
namespace pcl {
struct PCLPointCloud2 { PCLHeader header; };
struct PCLException : public std::runtime_error { PCLException(const std::string& s) : std::runtime_error(s) {} };
template <class T> inline void fromPCLPointCloud2(const PCLPointCloud2& in, PointCloud<T>& out) { out.header = in.header; out.points.clear(); }
}  // namespace pcl
namespace pcl_conversions {
inline void toPCL(const sensor_msgs::PointCloud2& in, pcl::PCLPointCloud2& out) { toPCL(in.header, out.header); }
}  // namespace pcl_conversions
namespace pcl_ros {
template <class T> inline bool transformPointCloud(const std::string&, const pcl::PointCloud<T>& in, pcl::PointCloud<T>& out, const tf::TransformListener&) {
  if (&in != &out) out = in;
  return true;
}
}  // namespace pcl_ros
