// Stand-in for <boost/thread.hpp>, for tools/tp_reference_harness.cpp only, over the standard library and written from Boost.Thread's
// documentation, as tools/dwa_ref_stubs has it - with one addition: boost::mutex tells the harness when it is unlocked.
// TrajectoryPlanner::generateTrajectory holds configuration_mutex_ for its whole body, so the unlock is the moment its output
// argument is complete.  The harness has one thread.
#pragma once
#include <mutex>
#include <thread>
#include <condition_variable>
#include <boost/shared_ptr.hpp>
#include <boost/function.hpp>
#include <boost/bind.hpp>
namespace tp_ref {
typedef void (*unlock_hook_t)();
inline unlock_hook_t& unlock_hook() { static unlock_hook_t h = nullptr; return h; }
}  // namespace tp_ref
namespace boost {
template <class M> using unique_lock = std::unique_lock<M>;
template <class M> using lock_guard = std::lock_guard<M>;
template <class M> using shared_lock = std::unique_lock<M>;
class mutex {
 public:
  typedef std::unique_lock<mutex> scoped_lock;
  void lock() { m_.lock(); }
  bool try_lock() { return m_.try_lock(); }
  void unlock() { if (tp_ref::unlock_hook()) tp_ref::unlock_hook()(); m_.unlock(); }
 private:
  std::mutex m_;
};
class recursive_mutex : public std::recursive_mutex { public: typedef std::unique_lock<recursive_mutex> scoped_lock; };
typedef recursive_mutex shared_mutex;
using std::thread; using std::condition_variable; using std::condition_variable_any;
namespace this_thread { inline void yield() {} }
}  // namespace boost
