// navgpu::AMCLOdom - amcl::AMCLOdom whose UpdateAction runs on the GPU (libnavgpu.so, navgpu_amcl_update_action).
//
// Drop-in for amcl_node: the node constructs this class where it constructs amcl::AMCLOdom (`odom_ = new AMCLOdom()`,
// amcl_node.cpp:679 and :980) and holds it as navgpu::AMCLOdom*, so that its SetModel calls (:681, :982) reach the shadows
// below; the odom_->UpdateAction call at :1464 then runs on the device.  The model and the alphas are private in the base class (amcl_odom.h:92-101): each shadow calls the base method and
// records the values for the device.
//
// UpdateAction(pf, data) replaces AMCLOdom::UpdateAction (amcl_odom.cpp:128-379): it uploads pf's
// current sample set, moves it on the device in the reference's drand48 mode, starting from this process's own drand48() state,
// writes the poses back and leaves the process's drand48 state where the reference's pf_ran_gaussian calls would have left it.
// The host's later drand48() calls (a host resample, randomFreeSpacePose) then continue the reference's stream exactly.  The
// state is read without consuming a draw through seed48's previous-state buffer and restored at once (drand48State).
// Poses agree with the reference's up to the device's sin / cos / atan2 / log (an ulp; see include/navgpu.h).
//
// There is no CPU fallback: the constructor throws navgpu::AmclError (status NAVGPU_ERR_NO_DEVICE) without a usable GPU, and
// any failing call throws with the library's status and message.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "amcl/pf/pf.h"
#include "amcl/sensors/amcl_odom.h"
#include "navgpu.h"
#include "navgpu_amcl_laser.h"  // navgpu::AmclError

namespace navgpu {

class AMCLOdom : public amcl::AMCLOdom {
 public:
  // max_samples: the first device capacity (amcl's max_particles default); a larger sample set grows it.
  explicit AMCLOdom(int max_samples = 5000, int device = 0);
  ~AMCLOdom() override = default;

  void SetModelDiff(double alpha1, double alpha2, double alpha3, double alpha4);
  void SetModelOmni(double alpha1, double alpha2, double alpha3, double alpha4, double alpha5);
  void SetModelGaussian(double alpha1, double alpha2, double alpha3, double alpha4, double alpha5);
  void SetModel(amcl::odom_model_t type, double alpha1, double alpha2, double alpha3, double alpha4, double alpha5 = 0);

  bool UpdateAction(pf_t* pf, amcl::AMCLSensorData* data) override;

  // The process's drand48() state X (48 bits), read through seed48 and restored: the next drand48() is unchanged.
  static uint64_t drand48State();
  static void setDrand48State(uint64_t x);

 private:
  struct Device;  // the navgpu_amcl handle and its capacity
  void ensureCapacity(int samples);

  std::shared_ptr<Device> dev_;
  int device_;
  navgpu_amcl_odom_params params_;
  bool configured_ = false;
  std::vector<double> poses_, weights_;
};

}  // namespace navgpu
