// Stand-in for <tf/message_filter.h>, for tools/costmap_reference_harness.cpp only, written from tf's documentation: the filter
// ObstacleLayer puts in front of a sensor topic, with the setTargetFrames the layer calls.  The harness configures no observation
// source, so no filter is ever created.
#pragma once
#include <string>
#include <vector>
#include <tf/transform_listener.h>
namespace tf {
class MessageFilterBase {
 public:
  virtual ~MessageFilterBase() {}
  virtual void clear() {}
  virtual void setTargetFrame(const std::string&) {}
  virtual void setTargetFrames(const std::vector<std::string>&) {}
  virtual void setTolerance(const ros::Duration&) {}
};
template <class M> class MessageFilter : public MessageFilterBase {
 public:
  template <class F> MessageFilter(F&, Transformer&, const std::string&, uint32_t) {}
  template <class C> void registerCallback(const C&) {}
};
}  // namespace tf
