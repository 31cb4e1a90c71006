// Stand-in for <pcl/point_cloud.h>, for tools/dwa_reference_harness.cpp only: the container DWAPlanner fills for its debug topics,
// written from PCL's documentation.  Nothing reads the clouds.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include <boost/shared_ptr.hpp>
namespace pcl {
struct PCLHeader { uint32_t seq; uint64_t stamp; std::string frame_id; PCLHeader() : seq(0), stamp(0) {} };
template <class T> struct PointCloud {
  PCLHeader header;
  std::vector<T> points;
  uint32_t width, height;
  bool is_dense;
  typedef boost::shared_ptr<PointCloud<T> > Ptr;
  typedef boost::shared_ptr<const PointCloud<T> > ConstPtr;
  PointCloud() : width(0), height(0), is_dense(true) {}
  size_t size() const { return points.size(); }
  void push_back(const T& p) { points.push_back(p); width = (uint32_t)points.size(); height = 1; }
  void clear() { points.clear(); width = height = 0; }
  T& operator[](size_t i) { return points[i]; }
  const T& operator[](size_t i) const { return points[i]; }
};
}  // namespace pcl
