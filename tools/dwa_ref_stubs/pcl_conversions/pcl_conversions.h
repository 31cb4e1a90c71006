// Stand-in for <pcl_conversions/pcl_conversions.h>, for tools/dwa_reference_harness.cpp only: the header conversions (PCL stamps are
// microseconds), written from the package's documentation.
#pragma once
#include <pcl/point_cloud.h>
#include <std_msgs/Header.h>
namespace pcl_conversions {
inline void fromPCL(const pcl::PCLHeader& in, std_msgs::Header& out) { out.seq = in.seq; out.stamp = ros::Time(in.stamp * 1e-6); out.frame_id = in.frame_id; }
inline std_msgs::Header fromPCL(const pcl::PCLHeader& in) { std_msgs::Header h; fromPCL(in, h); return h; }
inline void toPCL(const std_msgs::Header& in, pcl::PCLHeader& out) { out.seq = in.seq; out.stamp = (uint64_t)(in.stamp.toSec() * 1e6); out.frame_id = in.frame_id; }
inline pcl::PCLHeader toPCL(const std_msgs::Header& in) { pcl::PCLHeader h; toPCL(in, h); return h; }
}  // namespace pcl_conversions
