// Stand-in for global_planner/planner_core.h, used only by tools/make_global_planner_goldens.py.  The reference's header declares
// GlobalPlanner itself and with it pulls in costmap_2d_ros, nav_core, dynamic_reconfigure and the message headers; its dijkstra.h,
// astar.h and gradient_path.cpp include it for two things only: the "unassigned cell" potential and the console macros.  With this
// directory ahead of the reference's include directory they find this file, and dijkstra.cpp, astar.cpp and gradient_path.cpp
// compile as they stand.  Written from what those three sources use; nothing here is taken from the reference.
#pragma once
#define POT_HIGH 1.0e10  // the potential of a cell no expansion has reached (a double literal, as the sources compare against)
#include <ros/console.h>  // tests/ros_stubs: ROS_DEBUG as a no-op
#include <global_planner/potential_calculator.h>
#include <global_planner/expander.h>
#include <global_planner/traceback.h>
