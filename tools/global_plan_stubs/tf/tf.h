// Stand-in for <tf/tf.h> for tools/global_plan_harness.cpp only: the two functions the reference's orientation_filter.cpp calls, with
// tf's published formulas (tf::Quaternion::setRPY with roll = pitch = 0; tf::Matrix3x3::setRotation + getEulerYPR's yaw).  tf is not
// part of the reference tree; these are restated from its documentation.  Placed before tests/ros_stubs on the include path (whose
// tf.h returns zeros and serves the syntax check only).
#pragma once
#include <cmath>
#include <geometry_msgs/PoseStamped.h>
#include <geometry_msgs/Quaternion.h>
namespace tf {
inline geometry_msgs::Quaternion createQuaternionMsgFromYaw(double yaw) {
  const double half = yaw * 0.5;  // setRPY(0, 0, yaw): cos / sin of the zero half angles are 1 / 0, the products collapse
  geometry_msgs::Quaternion q;
  q.x = 0.0;
  q.y = 0.0;
  q.z = std::sin(half);
  q.w = std::cos(half);
  return q;
}
inline double getYaw(const geometry_msgs::Quaternion& m) {
  double x = m.x, y = m.y, z = m.z, w = m.w;
  const double len2 = x * x + y * y + z * z + w * w;
  if (std::fabs(len2 - 1.0) > 0.1) {  // quaternionMsgToTF: QUATERNION_TOLERANCE
    const double len = std::sqrt(len2);
    x /= len, y /= len, z /= len, w /= len;
  }
  const double d = x * x + y * y + z * z + w * w;  // Matrix3x3::setRotation
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, zz = z * zs;
  const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy;
  if (std::fabs(m20) >= 1.0) return 0.0;  // getEulerYPR's gimbal-lock branch: yaw = 0
  const double pitch = -std::asin(m20);
  return std::atan2(m10 / std::cos(pitch), m00 / std::cos(pitch));
}
}  // namespace tf
