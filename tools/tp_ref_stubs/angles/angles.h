// Working stand-in for <angles/angles.h> (the package is not in the reference tree), for tools/tp_reference_harness.cpp only, written from
// the package's documentation: normalize_angle_positive is the double fmod into [0, 2 pi), normalize_angle folds that into (-pi, pi],
// shortest_angular_distance(from, to) is normalize_angle(to - from).  Goes before tests/ros_stubs on the include path (whose angles.h
// serves a syntax check only and does not normalise).
#pragma once
#include <cmath>
namespace angles {
inline double from_degrees(double d) { return d * M_PI / 180.0; }
inline double to_degrees(double r) { return r * 180.0 / M_PI; }
inline double normalize_angle_positive(double a) { return fmod(fmod(a, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI); }
inline double normalize_angle(double a) {
  double r = normalize_angle_positive(a);
  if (r > M_PI) r -= 2.0 * M_PI;
  return r;
}
inline double shortest_angular_distance(double from, double to) { return normalize_angle(to - from); }
}  // namespace angles
