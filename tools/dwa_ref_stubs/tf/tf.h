// Working stand-in for <tf/tf.h>, for tools/dwa_reference_harness.cpp only, written from tf's documentation (LinearMath): what
// DWAPlanner, LocalPlannerUtil and goal_functions.cpp name.  A Transform keeps its rotation as the quaternion it was given (tf keeps
// the 3 x 3 basis; for the planar poses used here the yaw that comes back is the same float).  Yaw extraction follows
// Matrix3x3::setRotation + getEulerYPR.  Composing transforms is declared for the parts of goal_functions.cpp the harness never calls
// (they need a TransformListener) and covers planar transforms only.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <ros/time.h>
#include <geometry_msgs/PoseStamped.h>
#include <geometry_msgs/Quaternion.h>
namespace tf {
struct Vector3 {
  double v[3];
  Vector3(double x = 0, double y = 0, double z = 0) { v[0] = x; v[1] = y; v[2] = z; }
  double getX() const { return v[0]; } double getY() const { return v[1]; } double getZ() const { return v[2]; }
  double x() const { return v[0]; } double y() const { return v[1]; } double z() const { return v[2]; }
  void setX(double a) { v[0] = a; } void setY(double a) { v[1] = a; } void setZ(double a) { v[2] = a; }
  double length() const { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
  Vector3 operator-(const Vector3& o) const { return Vector3(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
  Vector3 operator+(const Vector3& o) const { return Vector3(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
};
typedef Vector3 Point;
struct Quaternion {
  double q[4];  // x, y, z, w
  Quaternion(double x = 0, double y = 0, double z = 0, double w = 1) { q[0] = x; q[1] = y; q[2] = z; q[3] = w; }
  double x() const { return q[0]; } double y() const { return q[1]; } double z() const { return q[2]; } double w() const { return q[3]; }
  void setRPY(double roll, double pitch, double yaw) {
    const double hy = yaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
    const double cy = std::cos(hy), sy = std::sin(hy), cp = std::cos(hp), sp = std::sin(hp), cr = std::cos(hr), sr = std::sin(hr);
    q[0] = sr * cp * cy - cr * sp * sy;
    q[1] = cr * sp * cy + sr * cp * sy;
    q[2] = cr * cp * sy - sr * sp * cy;
    q[3] = cr * cp * cy + sr * sp * sy;
  }
  double getAngle() const { return 2.0 * std::acos(q[3]); }
};
inline double yawOf(double x, double y, double z, double w) {  // Matrix3x3::setRotation, then getEulerYPR's yaw
  const double d = x * x + y * y + z * z + w * w;
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, zz = z * zs;
  const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy;
  (void)xx;
  if (std::fabs(m20) >= 1.0) return 0.0;
  const double pitch = -std::asin(m20);
  return std::atan2(m10 / std::cos(pitch), m00 / std::cos(pitch));
}
struct Matrix3x3 {
  Quaternion r;
  Matrix3x3() {}
  Matrix3x3(const Quaternion& q) : r(q) {}
  void setRotation(const Quaternion& q) { r = q; }
  void getEulerYPR(double& yaw, double& pitch, double& roll) const { yaw = yawOf(r.q[0], r.q[1], r.q[2], r.q[3]); pitch = roll = 0; }
  void getRPY(double& roll, double& pitch, double& yaw) const { getEulerYPR(yaw, pitch, roll); }
};
struct Transform {
  Vector3 o;
  Quaternion r;
  Transform() {}
  Transform(const Quaternion& q, const Vector3& v = Vector3()) : o(v), r(q) {}
  const Vector3& getOrigin() const { return o; }
  Vector3& getOrigin() { return o; }
  Quaternion getRotation() const { return r; }
  Matrix3x3 getBasis() const { return Matrix3x3(r); }
  void setOrigin(const Vector3& v) { o = v; }
  void setRotation(const Quaternion& q) { r = q; }
  void setBasis(const Matrix3x3& m) { r = m.r; }
  void setIdentity() { o = Vector3(); r = Quaternion(); }
  Vector3 operator*(const Vector3& p) const {
    const double yaw = yawOf(r.q[0], r.q[1], r.q[2], r.q[3]), c = std::cos(yaw), s = std::sin(yaw);
    return Vector3(o.v[0] + c * p.v[0] - s * p.v[1], o.v[1] + s * p.v[0] + c * p.v[1], o.v[2] + p.v[2]);
  }
  Transform operator*(const Transform& t) const {
    Quaternion q;
    q.setRPY(0, 0, yawOf(r.q[0], r.q[1], r.q[2], r.q[3]) + yawOf(t.r.q[0], t.r.q[1], t.r.q[2], t.r.q[3]));
    return Transform(q, (*this) * t.o);
  }
  Transform inverse() const {
    const double yaw = yawOf(r.q[0], r.q[1], r.q[2], r.q[3]), c = std::cos(yaw), s = std::sin(yaw);
    Quaternion q;
    q.setRPY(0, 0, -yaw);
    return Transform(q, Vector3(-(c * o.v[0] + s * o.v[1]), -(-s * o.v[0] + c * o.v[1]), -o.v[2]));
  }
};
typedef Transform Pose;
template <class T> struct Stamped : public T {
  ros::Time stamp_;
  std::string frame_id_;
  Stamped() {}
  Stamped(const T& t, const ros::Time& s, const std::string& f) : T(t), stamp_(s), frame_id_(f) {}
  void setData(const T& t) { *static_cast<T*>(this) = t; }
};
struct StampedTransform : public Transform { ros::Time stamp_; std::string frame_id_, child_frame_id_; };
inline double getYaw(const Quaternion& q) { return yawOf(q.q[0], q.q[1], q.q[2], q.q[3]); }
inline double getYaw(const geometry_msgs::Quaternion& m) {
  double x = m.x, y = m.y, z = m.z, w = m.w;
  const double len2 = x * x + y * y + z * z + w * w;
  if (std::fabs(len2 - 1.0) > 0.1) {  // quaternionMsgToTF normalises what is far from unit length
    const double len = std::sqrt(len2);
    x /= len, y /= len, z /= len, w /= len;
  }
  return yawOf(x, y, z, w);
}
inline Quaternion createQuaternionFromRPY(double r, double p, double y) { Quaternion q; q.setRPY(r, p, y); return q; }
inline Quaternion createQuaternionFromYaw(double yaw) { return createQuaternionFromRPY(0, 0, yaw); }
inline Quaternion createIdentityQuaternion() { return Quaternion(); }
inline geometry_msgs::Quaternion createQuaternionMsgFromYaw(double yaw) {
  const Quaternion q = createQuaternionFromYaw(yaw);
  geometry_msgs::Quaternion m;
  m.x = q.q[0], m.y = q.q[1], m.z = q.q[2], m.w = q.q[3];
  return m;
}
inline void quaternionMsgToTF(const geometry_msgs::Quaternion& m, Quaternion& q) { q = Quaternion(m.x, m.y, m.z, m.w); }
inline void poseMsgToTF(const geometry_msgs::Pose& m, Pose& p) {
  p.setOrigin(Vector3(m.position.x, m.position.y, m.position.z));
  Quaternion q;
  quaternionMsgToTF(m.orientation, q);
  p.setRotation(q);
}
inline void poseTFToMsg(const Pose& p, geometry_msgs::Pose& m) {
  m.position.x = p.o.v[0], m.position.y = p.o.v[1], m.position.z = p.o.v[2];
  m.orientation.x = p.r.q[0], m.orientation.y = p.r.q[1], m.orientation.z = p.r.q[2], m.orientation.w = p.r.q[3];
}
inline void poseStampedMsgToTF(const geometry_msgs::PoseStamped& m, Stamped<Pose>& p) {
  poseMsgToTF(m.pose, p);
  p.stamp_ = m.header.stamp;
  p.frame_id_ = m.header.frame_id;
}
inline void poseStampedTFToMsg(const Stamped<Pose>& p, geometry_msgs::PoseStamped& m) {
  poseTFToMsg(p, m.pose);
  m.header.stamp = p.stamp_;
  m.header.frame_id = p.frame_id_;
}
struct TransformException : public std::runtime_error { TransformException(const std::string& s) : std::runtime_error(s) {} };
typedef TransformException LookupException;
typedef TransformException ConnectivityException;
typedef TransformException ExtrapolationException;
}  // namespace tf
