// SYNTAX-CHECK STAND-IN for a ROS header that this image lacks (see ros/ros.h here).  Test infrastructure only.
#pragma once
#include <string>
#include <vector>
namespace dynamic_reconfigure {
struct DoubleParameter { std::string name; double value; };
struct Config { std::vector<DoubleParameter> doubles; };
struct Reconfigure { struct Request { Config config; } request; struct Response { Config config; } response; };
}
