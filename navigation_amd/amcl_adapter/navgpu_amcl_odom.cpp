// navgpu::AMCLOdom: see navgpu_amcl_odom.h.
#include "navgpu_amcl_odom.h"

#include <stdlib.h>

#include <algorithm>
#include <string>

namespace navgpu {

struct AMCLOdom::Device {
  navgpu_amcl* h = nullptr;
  int capacity = 0;
  ~Device() {
    if (h) navgpu_amcl_destroy(h);
  }
};

namespace {
void check(int rc, const char* what) {
  if (rc < 0) throw AmclError(rc, std::string(what) + ": " + navgpu_strerror(rc) + " " + navgpu_last_error());
}
}  // namespace

AMCLOdom::AMCLOdom(int max_samples, int device) : amcl::AMCLOdom(), device_(device), params_() {
  dev_ = std::make_shared<Device>();
  check(navgpu_amcl_create(1, (uint32_t)std::max(max_samples, 1), 1, device_, &dev_->h), "navgpu_amcl_create");
  dev_->capacity = std::max(max_samples, 1);
}

void AMCLOdom::SetModelDiff(double alpha1, double alpha2, double alpha3, double alpha4) {
  amcl::AMCLOdom::SetModelDiff(alpha1, alpha2, alpha3, alpha4);
  // SetModelDiff leaves alpha5 as it was; the diff models do not read it
  params_.model_type = NAVGPU_AMCL_ODOM_DIFF;
  params_.alpha1 = alpha1;
  params_.alpha2 = alpha2;
  params_.alpha3 = alpha3;
  params_.alpha4 = alpha4;
  configured_ = true;
}

void AMCLOdom::SetModelOmni(double alpha1, double alpha2, double alpha3, double alpha4, double alpha5) {
  amcl::AMCLOdom::SetModelOmni(alpha1, alpha2, alpha3, alpha4, alpha5);
  params_ = navgpu_amcl_odom_params{NAVGPU_AMCL_ODOM_OMNI, 0, alpha1, alpha2, alpha3, alpha4, alpha5};
  configured_ = true;
}

void AMCLOdom::SetModelGaussian(double alpha1, double alpha2, double alpha3, double alpha4, double alpha5) {
  amcl::AMCLOdom::SetModelGaussian(alpha1, alpha2, alpha3, alpha4, alpha5);
  params_ = navgpu_amcl_odom_params{NAVGPU_AMCL_ODOM_GAUSSIAN, 0, alpha1, alpha2, alpha3, alpha4, alpha5};
  configured_ = true;
}

void AMCLOdom::SetModel(amcl::odom_model_t type, double alpha1, double alpha2, double alpha3, double alpha4, double alpha5) {
  amcl::AMCLOdom::SetModel(type, alpha1, alpha2, alpha3, alpha4, alpha5);
  params_ = navgpu_amcl_odom_params{(int32_t)type, 0, alpha1, alpha2, alpha3, alpha4, alpha5};
  configured_ = true;
}

uint64_t AMCLOdom::drand48State() {
  unsigned short probe[3] = {0, 0, 0};
  const unsigned short* prev = seed48(probe);  // the previous state; the buffer is overwritten by the next seed48
  unsigned short saved[3] = {prev[0], prev[1], prev[2]};
  seed48(saved);
  return (uint64_t)saved[0] | (uint64_t)saved[1] << 16 | (uint64_t)saved[2] << 32;
}

void AMCLOdom::setDrand48State(uint64_t x) {
  unsigned short s[3] = {(unsigned short)(x & 0xFFFF), (unsigned short)(x >> 16 & 0xFFFF), (unsigned short)(x >> 32 & 0xFFFF)};
  seed48(s);
}

void AMCLOdom::ensureCapacity(int samples) {
  if (samples <= dev_->capacity) return;
  auto d = std::make_shared<Device>();
  check(navgpu_amcl_create(1, (uint32_t)samples, 1, device_, &d->h), "navgpu_amcl_create");
  d->capacity = samples;
  dev_ = d;
}

bool AMCLOdom::UpdateAction(pf_t* pf, amcl::AMCLSensorData* data) {
  if (!configured_) throw AmclError(NAVGPU_ERR_STATE, "navgpu::AMCLOdom::UpdateAction before a SetModel* call");
  const amcl::AMCLOdomData* od = static_cast<const amcl::AMCLOdomData*>(data);
  pf_sample_set_t* set = pf->sets + pf->current_set;
  const int n = set->sample_count;
  ensureCapacity(n);
  navgpu_amcl* h = dev_->h;
  check(navgpu_amcl_odom_configure(h, &params_), "navgpu_amcl_odom_configure");
  const size_t cap = (size_t)dev_->capacity;
  poses_.assign(cap * 3, 0.0);
  weights_.assign(cap, 0.0);
  for (int j = 0; j < n; ++j) {
    std::copy(set->samples[j].pose.v, set->samples[j].pose.v + 3, &poses_[3 * (size_t)j]);
    weights_[j] = set->samples[j].weight;
  }
  const int32_t count = n, converged = set->converged;
  check(navgpu_amcl_set_samples(h, 0, 1, &count, poses_.data(), weights_.data(), &converged), "navgpu_amcl_set_samples");
  double odom[9];
  std::copy(od->pose.v, od->pose.v + 3, odom);
  std::copy(od->delta.v, od->delta.v + 3, odom + 3);
  std::copy(od->absolute_motion.v, od->absolute_motion.v + 3, odom + 6);
  uint64_t state = drand48State();
  int32_t status = 0;
  check(navgpu_amcl_update_action(h, 0, 1, odom, NAVGPU_AMCL_DRAW_DRAND48, &state, 0, &status), "navgpu_amcl_update_action");
  check(navgpu_amcl_get_samples(h, 0, 1, nullptr, poses_.data(), nullptr, nullptr), "navgpu_amcl_get_samples");
  for (int j = 0; j < n; ++j) std::copy(&poses_[3 * (size_t)j], &poses_[3 * (size_t)j] + 3, set->samples[j].pose.v);
  setDrand48State(state);
  return true;
}

}  // namespace navgpu
