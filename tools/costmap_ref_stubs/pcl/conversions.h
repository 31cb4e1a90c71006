// Stand-in for <pcl/conversions.h>, for tools/costmap_reference_harness.cpp only: see pcl_ros/transforms.h beside it.
#pragma once
#include <pcl_ros/transforms.h>
