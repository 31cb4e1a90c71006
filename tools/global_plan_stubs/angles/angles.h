// Stand-in for <angles/angles.h> for tools/global_plan_harness.cpp only: the published fmod form of normalize_angle (the package is
// not part of the reference tree).
#pragma once
#include <cmath>
namespace angles {
inline double normalize_angle_positive(double angle) { return std::fmod(std::fmod(angle, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI); }
inline double normalize_angle(double angle) {
  double a = normalize_angle_positive(angle);
  if (a > M_PI) a -= 2.0 * M_PI;
  return a;
}
inline double shortest_angular_distance(double from, double to) { return normalize_angle(to - from); }
}  // namespace angles
