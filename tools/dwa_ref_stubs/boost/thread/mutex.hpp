// See ../thread.hpp.
#pragma once
#include <boost/thread.hpp>
