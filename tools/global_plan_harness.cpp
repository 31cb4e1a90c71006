// Runs plans through the reference's own OrientationFilter::processPath (global_planner/src/orientation_filter.cpp, compiled in place
// by tools/make_global_plan_goldens.py) in its four modes and writes the quaternions it leaves.  tf and angles come from
// tools/global_plan_stubs/ (their formulas), the message types from tests/ros_stubs/.
//   in : int64 n_plans; per plan: int64 n, double start_yaw, n x {x, y, yaw}
//   out: per plan, per mode 0..3: n x {z, w}
#include <cstdint>
#include <cstdio>
#include <vector>

#include <global_planner/orientation_filter.h>
#include <tf/tf.h>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t n_plans = 0;
  if (fread(&n_plans, sizeof n_plans, 1, in) != 1) return 3;
  for (int64_t p = 0; p < n_plans; ++p) {
    int64_t n = 0;
    double start_yaw = 0;
    if (fread(&n, sizeof n, 1, in) != 1 || fread(&start_yaw, sizeof start_yaw, 1, in) != 1) return 3;
    std::vector<double> xyyaw(3 * n);
    if (fread(xyyaw.data(), sizeof(double), xyyaw.size(), in) != xyyaw.size()) return 3;
    geometry_msgs::PoseStamped start;
    start.pose.orientation = tf::createQuaternionMsgFromYaw(start_yaw);
    for (int mode = 0; mode < 4; ++mode) {
      std::vector<geometry_msgs::PoseStamped> path(n);
      for (int64_t i = 0; i < n; ++i) {
        path[i].pose.position.x = xyyaw[3 * i];
        path[i].pose.position.y = xyyaw[3 * i + 1];
        // getPlanFromPotential writes the identity; a goal pose carries the caller's orientation
        if (xyyaw[3 * i + 2] != 0.0) path[i].pose.orientation = tf::createQuaternionMsgFromYaw(xyyaw[3 * i + 2]);
      }
      global_planner::OrientationFilter filter;
      filter.setMode(mode);
      if (!(mode == 3 && n < 3)) filter.processPath(start, path);  // (there the reference reads before its array)
      for (int64_t i = 0; i < n; ++i) {
        const double zw[2] = {path[i].pose.orientation.z, path[i].pose.orientation.w};
        fwrite(zw, sizeof(double), 2, out);
      }
    }
  }
  fclose(out);
  fclose(in);
  return 0;
}
