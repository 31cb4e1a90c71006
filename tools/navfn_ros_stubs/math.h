// <math.h> as navfn.h (navfn/include/navfn/navfn.h:44) meant it: the C header.  libstdc++ from GCC 6 on ships a math.h of its own
// that also brings std::hypot(float, float) and its kin into the global namespace, which turns NavFn's `hypot(x, y)` on floats
// (navfn.cpp:962, 1046) from C's hypot(double, double) - what the toolchains the reference was written for compile, and what the
// library and the CPU oracle restate - into hypotf: path points then differ in the last bit here and there.  This header goes
// straight to the C one, the way <cmath> itself does.  Used only by tools/make_navfn_ros_goldens.py.
#pragma once
#define _GLIBCXX_INCLUDE_NEXT_C_HEADERS
#include_next <math.h>
#undef _GLIBCXX_INCLUDE_NEXT_C_HEADERS
