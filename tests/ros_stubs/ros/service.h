// SYNTAX-CHECK STAND-IN for a ROS header that this image lacks (see ros/ros.h here).  Test infrastructure only.
#pragma once
#include <string>
namespace ros {
struct ServiceClient { template <class S> bool call(S&) { return true; } bool isValid() const { return true; } };
namespace service { template <class S> ServiceClient createClient(const std::string&, bool = false) { return ServiceClient(); } }
}
