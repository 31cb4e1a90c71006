// SYNTAX-CHECK STAND-IN for a ROS / Boost / PCL / Eigen header that this image lacks.  Test infrastructure only
// (tests/test_plugin_syntax.py): it lets g++ -fsyntax-only parse navigation_amd/plugin/*.cpp against the REFERENCE'S OWN
// headers.  No reference code is built with it, nothing is linked, nothing here is part of the product.
// (dynamic_reconfigure generates the real header from navfn/cfg/NavfnROS.cfg:14-36.)
#pragma once
namespace navfn { struct NavfnROSConfig { bool allow_unknown; double default_tolerance, tolerance_weight_dist_from_goal, tolerance_weight_path_length; NavfnROSConfig() : allow_unknown(true), default_tolerance(0.0), tolerance_weight_dist_from_goal(1.0), tolerance_weight_path_length(0.0) {} }; }
