// Stand-in for <boost/tokenizer.hpp>, for tools/dwa_reference_harness.cpp only: costmap_2d's footprint.cpp includes the header and
// uses nothing from it.
#pragma once
