// Adds what obstacle_layer.cpp and static_layer.cpp name to the <tf/tf.h> stand-in of tools/dwa_ref_stubs, for
// tools/costmap_reference_harness.cpp only: tf::getPrefixParam and tf::resolve (no prefix: a frame name stays as it is), and a
// StampedTransform that can be applied to a point.  The harness keeps every frame equal, so the transform StaticLayer's rolling branch
// looks up is the identity, and applying it returns the point unchanged.
#pragma once
#define StampedTransform StampedTransformData
#include_next <tf/tf.h>
#undef StampedTransform
#include <ros/ros.h>
namespace tf {
struct StampedTransform : public StampedTransformData {
  Point operator()(const Point& p) const { return p; }
};
inline std::string getPrefixParam(ros::NodeHandle&) { return std::string(); }
inline std::string resolve(const std::string&, const std::string& frame) { return frame; }
}  // namespace tf
