// Stand-in for <boost/thread.hpp>, for tools/dwa_reference_harness.cpp only, over the standard library: the mutex types with Boost's
// nested scoped_lock, written from Boost.Thread's documentation.  The harness has one thread.
#pragma once
#include <mutex>
#include <thread>
#include <condition_variable>
#include <boost/shared_ptr.hpp>
#include <boost/function.hpp>
#include <boost/bind.hpp>
namespace boost {
template <class M> using unique_lock = std::unique_lock<M>;
template <class M> using lock_guard = std::lock_guard<M>;
template <class M> using shared_lock = std::unique_lock<M>;
class mutex : public std::mutex { public: typedef std::unique_lock<mutex> scoped_lock; };
class recursive_mutex : public std::recursive_mutex { public: typedef std::unique_lock<recursive_mutex> scoped_lock; };
typedef recursive_mutex shared_mutex;
using std::thread; using std::condition_variable; using std::condition_variable_any;
namespace this_thread { inline void yield() {} }
}  // namespace boost
