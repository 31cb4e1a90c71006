// Working stand-in for <ros/ros.h>, for tools/dwa_reference_harness.cpp only, written from roscpp's documentation: a NodeHandle whose
// parameters live in one process-wide table that the harness fills (dwa_ref::params()), names compared by their last component, and an
// XmlRpcValue that converts the way footprint.cpp asks.  Publishers and subscribers do nothing.
#pragma once
#include <cmath>
#include <cstring>
#include <climits>
#include <cfloat>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include <stdexcept>
#include <stdint.h>
#include <boost/shared_ptr.hpp>
#include <boost/function.hpp>
#include <boost/bind.hpp>
#include <ros/console.h>
#include <ros/assert.h>
#include <ros/time.h>
namespace dwa_ref {
inline std::map<std::string, double>& params() { static std::map<std::string, double> p; return p; }
inline std::string leaf(const std::string& n) { size_t k = n.rfind('/'); return k == std::string::npos ? n : n.substr(k + 1); }
inline void assign(bool& v, double d) { v = d != 0.0; }
inline void assign(int& v, double d) { v = (int)d; }
inline void assign(double& v, double d) { v = d; }
template <class T> inline void assign(T&, double) {}
}  // namespace dwa_ref
namespace XmlRpc {
class XmlRpcValue {
 public:
  enum Type { TypeInvalid, TypeArray, TypeString, TypeDouble, TypeInt, TypeStruct };
  typedef std::map<std::string, XmlRpcValue> ValueStruct;
  typedef std::vector<XmlRpcValue> ValueArray;
  XmlRpcValue() : _type(TypeInvalid), number_(0), int_(0) { _value.asStruct = 0; }
  Type getType() const { return _type; }
  int size() const { return (int)array_.size(); }
  XmlRpcValue& operator[](int i) { return array_[i]; }
  XmlRpcValue& operator[](const char* k) { return struct_[k]; }
  bool hasMember(const std::string& k) const { return struct_.count(k) != 0; }
  operator double&() { return number_; }
  operator int&() { int_ = (int)number_; return int_; }
  operator std::string&() { return string_; }
 protected:  // the two members costmap_2d_ros.h's SuperValue sets
  Type _type;
  union { ValueStruct* asStruct; ValueArray* asArray; } _value;
 private:
  double number_;
  int int_;
  std::string string_;
  std::vector<XmlRpcValue> array_;
  std::map<std::string, XmlRpcValue> struct_;
};
}  // namespace XmlRpc
namespace ros {
struct Publisher { template <class M> void publish(const M&) const {} uint32_t getNumSubscribers() const { return 0; } void shutdown() {} operator bool() const { return true; } };
struct Subscriber { void shutdown() {} std::string getTopic() const { return std::string(); } };
struct Timer { void stop() {} void start() {} };
struct TimerEvent {};
struct SingleSubscriberPublisher {};
class NodeHandle {
 public:
  NodeHandle() {}
  NodeHandle(const std::string&) {}
  NodeHandle(const NodeHandle&, const std::string&) {}
  template <class T> bool getParam(const std::string& n, T& v) const {
    std::map<std::string, double>::const_iterator it = dwa_ref::params().find(dwa_ref::leaf(n));
    if (it == dwa_ref::params().end()) return false;
    dwa_ref::assign(v, it->second);
    return true;
  }
  template <class T> bool param(const std::string& n, T& v, const T& d) const { if (getParam(n, v)) return true; v = d; return false; }
  template <class T> void setParam(const std::string&, const T&) const {}
  bool hasParam(const std::string& n) const { return dwa_ref::params().count(dwa_ref::leaf(n)) != 0; }
  bool searchParam(const std::string& n, std::string& found) const { if (!hasParam(n)) return false; found = n; return true; }
  bool deleteParam(const std::string&) const { return false; }
  std::string getNamespace() const { return std::string(); }
  std::string resolveName(const std::string& n) const { return n; }
  template <class M> Publisher advertise(const std::string&, uint32_t, bool = false) { return Publisher(); }
  template <class M, class C> Publisher advertise(const std::string&, uint32_t, const C&) { return Publisher(); }
  template <class M, class T> Subscriber subscribe(const std::string&, uint32_t, void (T::*)(const boost::shared_ptr<M const>&), T*) { return Subscriber(); }
  template <class M> Subscriber subscribe(const std::string&, uint32_t, const boost::function<void(const boost::shared_ptr<M const>&)>&) { return Subscriber(); }
  template <class T> Timer createTimer(Duration, void (T::*)(const TimerEvent&), T*, bool = false) { return Timer(); }
  bool ok() const { return true; }
};
inline bool ok() { return true; }
inline void spinOnce() {}
namespace this_node { inline std::string getName() { return std::string(); } }
}  // namespace ros
