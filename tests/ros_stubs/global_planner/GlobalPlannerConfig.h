// SYNTAX-CHECK STAND-IN for a ROS / Boost / PCL / Eigen header that this image lacks.  Test infrastructure only
// (tests/test_plugin_syntax.py): it lets g++ -fsyntax-only parse navigation_amd/plugin/*.cpp against the REFERENCE'S OWN
// headers.  No reference code is built with it, nothing is linked, nothing here is part of the product.
// (dynamic_reconfigure generates the real header from global_planner/cfg/GlobalPlanner.cfg:8-21.)
#pragma once
namespace global_planner { struct GlobalPlannerConfig { int lethal_cost, neutral_cost, orientation_mode; double cost_factor; bool publish_potential, restore_defaults; GlobalPlannerConfig() : lethal_cost(253), neutral_cost(50), orientation_mode(1), cost_factor(3.0), publish_potential(true), restore_defaults(false) {} }; }
