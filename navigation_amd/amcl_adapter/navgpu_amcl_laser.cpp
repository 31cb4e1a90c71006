// navgpu::AMCLLaser: see navgpu_amcl_laser.h.
#include "navgpu_amcl_laser.h"

#include <algorithm>

namespace navgpu {

struct AMCLLaser::Device {
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

AMCLLaser::AMCLLaser(size_t max_beams, map_t* map, int max_samples, int device)
    : amcl::AMCLLaser(max_beams, map), map_(map), max_beams_((int)max_beams), device_(device), params_() {
  // the reference's defaults: the model is set by a SetModel* call, the map factors by the constructor (amcl_laser.cpp:51-53)
  params_.max_beams = max_beams_;
  params_.off_map_factor = 1.0;
  params_.non_free_space_factor = 1.0;
  params_.non_free_space_radius = 0.0;
  dev_ = std::make_shared<Device>();
  check(navgpu_amcl_create(1, (uint32_t)std::max(max_samples, 1), (uint32_t)std::max(max_beams_, 1), device_, &dev_->h), "navgpu_amcl_create");
  dev_->capacity = std::max(max_samples, 1);
}

AMCLLaser::AMCLLaser(const AMCLLaser& o)
    : amcl::AMCLLaser(o), dev_(o.dev_), map_(o.map_), max_beams_(o.max_beams_), device_(o.device_), params_(o.params_),
      max_occ_dist_(o.max_occ_dist_), map_dirty_(true) {
  std::copy(o.laser_pose_, o.laser_pose_ + 3, laser_pose_);
}

void AMCLLaser::SetModelBeam(double z_hit, double z_short, double z_max, double z_rand, double sigma_hit, double lambda_short,
                             double chi_outlier) {
  amcl::AMCLLaser::SetModelBeam(z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short, chi_outlier);
  params_.model_type = NAVGPU_AMCL_MODEL_BEAM;
  params_.z_hit = z_hit;
  params_.z_short = z_short;
  params_.z_max = z_max;
  params_.z_rand = z_rand;
  params_.sigma_hit = sigma_hit;
  params_.lambda_short = lambda_short;
  params_.chi_outlier = chi_outlier;
  map_dirty_ = true;
}

void AMCLLaser::SetModelLikelihoodField(double z_hit, double z_rand, double sigma_hit, double max_occ_dist) {
  amcl::AMCLLaser::SetModelLikelihoodField(z_hit, z_rand, sigma_hit, max_occ_dist);
  params_.model_type = NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD;
  params_.z_hit = z_hit;
  params_.z_rand = z_rand;
  params_.sigma_hit = sigma_hit;
  max_occ_dist_ = max_occ_dist;
  map_dirty_ = true;
}

void AMCLLaser::SetModelLikelihoodFieldProb(double z_hit, double z_rand, double sigma_hit, double max_occ_dist, bool do_beamskip,
                                            double beam_skip_distance, double beam_skip_threshold, double beam_skip_error_threshold) {
  amcl::AMCLLaser::SetModelLikelihoodFieldProb(z_hit, z_rand, sigma_hit, max_occ_dist, do_beamskip, beam_skip_distance, beam_skip_threshold,
                                               beam_skip_error_threshold);
  params_.model_type = NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB;
  params_.z_hit = z_hit;
  params_.z_rand = z_rand;
  params_.sigma_hit = sigma_hit;
  params_.do_beamskip = do_beamskip ? 1 : 0;
  params_.beam_skip_distance = beam_skip_distance;
  params_.beam_skip_threshold = beam_skip_threshold;
  params_.beam_skip_error_threshold = beam_skip_error_threshold;
  max_occ_dist_ = max_occ_dist;
  map_dirty_ = true;
}

void AMCLLaser::SetModelLikelihoodFieldGompertz(double z_hit, double z_rand, double sigma_hit, double max_occ_dist, double gompertz_a,
                                                double gompertz_b, double gompertz_c, double input_shift, double input_scale,
                                                double output_shift) {
  amcl::AMCLLaser::SetModelLikelihoodFieldGompertz(z_hit, z_rand, sigma_hit, max_occ_dist, gompertz_a, gompertz_b, gompertz_c, input_shift,
                                                   input_scale, output_shift);
  params_.model_type = NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_GOMPERTZ;
  params_.z_hit = z_hit;
  params_.z_rand = z_rand;
  params_.sigma_hit = sigma_hit;
  params_.gompertz_a = gompertz_a;
  params_.gompertz_b = gompertz_b;
  params_.gompertz_c = gompertz_c;
  params_.input_shift = input_shift;
  params_.input_scale = input_scale;
  params_.output_shift = output_shift;
  max_occ_dist_ = max_occ_dist;
  map_dirty_ = true;
}

void AMCLLaser::SetMapFactors(double off_map_factor, double non_free_space_factor, double non_free_space_radius) {
  amcl::AMCLLaser::SetMapFactors(off_map_factor, non_free_space_factor, non_free_space_radius);
  params_.off_map_factor = off_map_factor;
  params_.non_free_space_factor = non_free_space_factor;
  params_.non_free_space_radius = non_free_space_radius;
}

void AMCLLaser::SetLaserPose(pf_vector_t& laser_pose) {
  amcl::AMCLLaser::SetLaserPose(laser_pose);
  std::copy(laser_pose.v, laser_pose.v + 3, laser_pose_);
}

void AMCLLaser::ensureCapacity(int samples) {
  if (samples <= dev_->capacity) return;
  auto d = std::make_shared<Device>();
  check(navgpu_amcl_create(1, (uint32_t)samples, (uint32_t)std::max(max_beams_, 1), device_, &d->h), "navgpu_amcl_create");
  d->capacity = samples;
  dev_ = d;  // copies made earlier keep the old handle
  map_dirty_ = true;
}

// The base class's map_t as it stands: occupancy, and the reference's own distances once a SetModelLikelihoodField* call has
// run map_update_cspace on it (the beam model's map keeps the device's exact transform)
void AMCLLaser::uploadMap() {
  const size_t cells = (size_t)map_->size_x * map_->size_y;
  std::vector<int8_t> occ(cells);
  for (size_t i = 0; i < cells; ++i) occ[i] = map_->cells[i].occ_state;
  const double max_occ_dist = map_->distances ? map_->max_occ_dist : max_occ_dist_;
  check(navgpu_amcl_set_map_cells(dev_->h, 0, 1, occ.data(), (uint32_t)map_->size_x, (uint32_t)map_->size_y, map_->scale, map_->origin_x,
                                  map_->origin_y, 1, max_occ_dist),
        "navgpu_amcl_set_map_cells");
  if (map_->distances) check(navgpu_amcl_set_distance_map(dev_->h, 0, 1, map_->distances, 1), "navgpu_amcl_set_distance_map");
  map_dirty_ = false;
}

bool AMCLLaser::UpdateSensor(pf_t* pf, amcl::AMCLSensorData* data) {
  if (max_beams_ < 2) return false;  // amcl_laser.cpp:163-164
  pf_sample_set_t* set = pf->sets + pf->current_set;
  const int n = set->sample_count;
  ensureCapacity(n);
  if (map_dirty_) uploadMap();
  navgpu_amcl* h = dev_->h;
  navgpu_amcl_laser_params p = params_;
  p.alpha_slow = pf->alpha_slow;
  p.alpha_fast = pf->alpha_fast;
  check(navgpu_amcl_laser_configure(h, &p), "navgpu_amcl_laser_configure");
  check(navgpu_amcl_set_laser_pose(h, 0, 1, laser_pose_), "navgpu_amcl_set_laser_pose");
  const size_t cap = (size_t)dev_->capacity;
  poses_.assign(cap * 3, 0.0);
  weights_.assign(cap, 0.0);
  for (int j = 0; j < n; ++j) {
    std::copy(set->samples[j].pose.v, set->samples[j].pose.v + 3, &poses_[3 * (size_t)j]);
    weights_[j] = set->samples[j].weight;
  }
  const int32_t count = n, converged = set->converged;
  check(navgpu_amcl_set_samples(h, 0, 1, &count, poses_.data(), weights_.data(), &converged), "navgpu_amcl_set_samples");
  double w[2] = {pf->w_slow, pf->w_fast};
  check(navgpu_amcl_set_filter_state(h, 0, 1, w), "navgpu_amcl_set_filter_state");
  const amcl::AMCLLaserData* ld = static_cast<const amcl::AMCLLaserData*>(data);
  const uint32_t rc = ld->range_count > 0 ? (uint32_t)ld->range_count : 0u;
  const double range_max = ld->range_max;
  int32_t updated = 0;
  check(navgpu_amcl_update_sensor(h, 0, 1, rc ? &ld->ranges[0][0] : nullptr, &rc, &range_max, &updated), "navgpu_amcl_update_sensor");
  if (updated != 1) return false;
  check(navgpu_amcl_get_samples(h, 0, 1, nullptr, nullptr, weights_.data(), nullptr), "navgpu_amcl_get_samples");
  check(navgpu_amcl_get_filter_state(h, 0, 1, w), "navgpu_amcl_get_filter_state");
  for (int j = 0; j < n; ++j) set->samples[j].weight = weights_[j];
  pf->w_slow = w[0];
  pf->w_fast = w[1];
  return true;
}

}  // namespace navgpu
