// navgpu::AMCLLaser - amcl::AMCLLaser whose UpdateSensor runs on the GPU (libnavgpu.so, navgpu_amcl_*).
//
// Drop-in for amcl_node: the node constructs this class where it constructs amcl::AMCLLaser (amcl_node.cpp:684, :985,
// and the per-laser copy at :1343) and holds it as navgpu::AMCLLaser* (the `laser_` / `lasers_` members, :198, :228), so that
// its SetModel* / SetMapFactors / SetLaserPose calls reach the shadows below.  The model parameters are private in the base
// class (amcl_laser.h:147-194): each shadow calls the base method and records the values for the device.
//
// UpdateSensor(pf, data) replaces AMCLLaser::UpdateSensor -> pf_update_sensor(pf, ApplyModelToSampleSet, data)
// (amcl_laser.cpp:160-167, pf.c:270-316): it uploads pf's current sample set, w_slow / w_fast and the scan, runs the update on
// the device and writes the weights, w_slow and w_fast back into pf.  The map (occupancy and, after SetModelLikelihoodField*,
// the reference's own map_t::distances) is uploaded on the first update after a SetModel* call.  Motion model, resampling and
// the kd-tree stay on the CPU, as does the static AMCLLaser::ApplyModelToSampleSet the node calls for a forced pose update.
//
// There is no CPU fallback: the constructor throws navgpu::AmclError (status NAVGPU_ERR_NO_DEVICE) without a usable GPU, and
// any failing call throws with the library's status and message.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "amcl/map/map.h"
#include "amcl/pf/pf.h"
#include "amcl/sensors/amcl_laser.h"
#include "navgpu.h"

namespace navgpu {

class AmclError : public std::runtime_error {
 public:
  AmclError(int status, const std::string& what) : std::runtime_error(what), status_(status) {}
  int status() const { return status_; }

 private:
  int status_;
};

class AMCLLaser : public amcl::AMCLLaser {
 public:
  // max_samples: the first device capacity (amcl's max_particles default); a larger sample set grows it.
  AMCLLaser(size_t max_beams, map_t* map, int max_samples = 5000, int device = 0);
  AMCLLaser(const AMCLLaser& other);  // copies share the device handle (amcl_node.cpp:1343 keeps one per laser)
  AMCLLaser& operator=(const AMCLLaser&) = delete;
  ~AMCLLaser() override = default;

  void SetModelBeam(double z_hit, double z_short, double z_max, double z_rand, double sigma_hit, double lambda_short, double chi_outlier);
  void SetModelLikelihoodField(double z_hit, double z_rand, double sigma_hit, double max_occ_dist);
  void SetModelLikelihoodFieldProb(double z_hit, double z_rand, double sigma_hit, double max_occ_dist, bool do_beamskip,
                                   double beam_skip_distance, double beam_skip_threshold, double beam_skip_error_threshold);
  void SetModelLikelihoodFieldGompertz(double z_hit, double z_rand, double sigma_hit, double max_occ_dist, double gompertz_a,
                                       double gompertz_b, double gompertz_c, double input_shift, double input_scale, double output_shift);
  void SetMapFactors(double off_map_factor, double non_free_space_factor, double non_free_space_radius);
  void SetLaserPose(pf_vector_t& laser_pose);

  bool UpdateSensor(pf_t* pf, amcl::AMCLSensorData* data) override;

 private:
  struct Device;  // the navgpu_amcl handle and its capacity
  void ensureCapacity(int samples);
  void uploadMap();

  std::shared_ptr<Device> dev_;
  map_t* map_;
  int max_beams_;
  int device_;
  navgpu_amcl_laser_params params_;
  double max_occ_dist_ = 0.0;  // of the last SetModelLikelihoodField*; the beam model's map gets map_t::max_occ_dist
  bool map_dirty_ = true;
  double laser_pose_[3] = {0.0, 0.0, 0.0};
  std::vector<double> poses_, weights_;
};

}  // namespace navgpu
