// Adds ros::names to the <ros/ros.h> stand-in of tools/dwa_ref_stubs, for tools/costmap_reference_harness.cpp only.  A name resolves
// to what that stand-in's Subscriber::getTopic() answers, the empty string: there is no master and nothing is ever subscribed.  With
// first_map_only set, StaticLayer::onInitialize therefore takes its map subscription as standing and does not wait for a map server;
// the harness then delivers the map through StaticLayer::incomingMap itself.
#pragma once
#include_next <ros/ros.h>
namespace ros {
namespace names {
inline std::string resolve(const std::string&) { return std::string(); }
}  // namespace names
}  // namespace ros
