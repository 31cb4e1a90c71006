// navgpu_amcl_node_*: AmclNode::laserReceived (amcl/src/amcl_node.cpp:1316-1756) for every filter of a slice in one call, and the
// node state it keeps between scans (include/navgpu.h).  The decisions are plain host arithmetic in the reference's own
// expressions; the pf steps are navgpu_amcl.cpp's step bodies (navgpu_amcl_host.h) with each filter predicated by what the node
// decided for it; the scan conversion and the hypothesis read-out are amcl_node_kernels.hip.  One wait per call.
#include "navgpu_amcl_host.h"

namespace {
struct NodeDecision {  // one flagged filter of a laser_received call
  bool refused = false, moved = false, updated = false, resampled = false, force_publication = false, cloud_due = false;
  double odom[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // AMCLOdomData: pose, delta, absolute_motion (amcl_node.cpp:1447-1453)
};

// amcl_node.cpp:1391-1440 and the bookkeeping of :1442-1470 and :1474-1562 that needs no pf result.  s is the filter's node
// state, changed as the reference changes it.
NodeDecision decide(const navgpu_amcl_node_params& N, navgpu_amcl_node_state& s, const double pose[3]) {
  NodeDecision d;
  double delta[3] = {0.0, 0.0, 0.0};  // pf_vector_zero()
  if (s.pf_init) {
    // Compute change in pose
    delta[0] = pose[0] - s.pf_odom_pose[0];
    delta[1] = pose[1] - s.pf_odom_pose[1];
    delta[2] = navgpu::amclAngleDiff(pose[2], s.pf_odom_pose[2]);
    // See if we should update the filter
    bool update;
    const double* am = s.odom_integrator_absolute_motion;
    if (N.use_odom_integrator) {
      const double abs_trans = sqrt(am[0] * am[0] + am[1] * am[1]);
      const double abs_rot = am[2];
      update = abs_trans >= N.d_thresh || abs_rot >= N.a_thresh;
    } else {
      update = fabs(delta[0]) > N.d_thresh || fabs(delta[1]) > N.d_thresh || fabs(delta[2]) > N.a_thresh;
    }
    update = update || s.force_update;
    s.force_update = 0;
    if (update) s.lasers_update = 1;
  }
  if (!s.pf_init) {
    std::copy(pose, pose + 3, s.pf_odom_pose);  // Pose at last filter update
    s.pf_init = 1;                              // Filter is now initialized
    s.lasers_update = 1;                        // Should update sensor data
    d.force_publication = true;
    s.resample_count = 0;
    s.odom_integrator_ready = 0;  // initOdomIntegrator()
  } else if (s.lasers_update) {   // If the robot has moved, update the filter
    d.moved = true;
    std::copy(pose, pose + 3, d.odom);
    std::copy(delta, delta + 3, d.odom + 3);
    std::copy(s.odom_integrator_absolute_motion, s.odom_integrator_absolute_motion + 3, d.odom + 6);
    std::fill(s.odom_integrator_absolute_motion, s.odom_integrator_absolute_motion + 3, 0.0);  // resetOdomIntegrator()
  }
  if (s.lasers_update) {
    d.updated = true;
    s.lasers_update = 0;
    std::copy(pose, pose + 3, s.pf_odom_pose);
    // ++ of an int: the reference's count wraps through signed overflow after 2^31 scans; here it wraps as unsigned does
    s.resample_count = (int32_t)((uint32_t)s.resample_count + 1u);
    if (!(s.resample_count % N.resample_interval)) d.resampled = true;
    d.cloud_due = !s.force_update;
  }
  return d;
}

// The scan's thresholds and angles (amcl_node.cpp:1505-1522) for k_amcl_scan; range_max is also AMCLLaserData::range_max
void convertScan(const navgpu_amcl_node_params& N, const navgpu_amcl_scan& m, navgpu::AmclScanDev& sc) {
  const double angle_min = m.yaw_min;
  double angle_increment = m.yaw_inc - angle_min;
  // wrapping angle to [-pi .. pi]
  angle_increment = fmod(angle_increment + 5 * M_PI, 2 * M_PI) - M_PI;
  // Apply range min/max thresholds, if the user supplied them
  double range_max, range_min;
  if (N.laser_max_range > 0.0)
    range_max = std::min(m.range_max, (float)N.laser_max_range);
  else
    range_max = m.range_max;
  if (N.laser_min_range > 0.0)
    range_min = std::max(m.range_min, (float)N.laser_min_range);
  else
    range_min = m.range_min;
  sc.range_off = m.range_offset;
  sc.range_count = (int32_t)m.range_count;
  sc.range_min = range_min;
  sc.range_max = range_max;
  sc.angle_min = angle_min;
  sc.angle_inc = angle_increment;
}

// The read-out of one filter into its result record, after the wait
void fillHypothesis(const navgpu_amcl* h, uint32_t f, const navgpu::AmclHypDev& H, navgpu_amcl_node_result& r) {
  r.cluster_count = H.clusters;
  r.max_weight_hyp = H.max_weight_hyp;
  r.max_weight = H.max_weight;
  r.published = H.max_weight > 0.0 ? 1 : 0;
  std::copy(H.pose, H.pose + 3, r.pose);
  r.cov_xx = H.cov[0];
  r.cov_xy = H.cov[1];
  r.cov_yx = H.cov[2];
  r.cov_yy = H.cov[3];
  r.cov_aa = H.cov[4];
  r.sample_count = h->sample_count[f];
  r.converged = h->converged[f];
}

// The records of the node's device pieces and the pinned staging of a call: [n] of each record type, then the read-back
struct NodeStage {
  navgpu::AmclOdomFilterDev* odom;
  navgpu::AmclFilterDev* filters;
  navgpu::AmclScanDev* scans;
  navgpu::AmclResampleFilterDev* resample;
  navgpu::AmclHypDev* hyps;
  navgpu::AmclResampleFilterDev* resample_back;
  navgpu::AmclHypDev* hyps_back;
};
constexpr size_t kStagePerFilter = sizeof(navgpu::AmclOdomFilterDev) + sizeof(navgpu::AmclFilterDev) + sizeof(navgpu::AmclScanDev) +
                                   2 * sizeof(navgpu::AmclResampleFilterDev) + 2 * sizeof(navgpu::AmclHypDev);

int nodeWorkspace(navgpu_amcl* h, NodeStage& st) {
  if (int rc = h->resampleWorkspace()) return rc;
  if (!h->d_hyps) {
    int rc = h->d_scans ? NAVGPU_OK : h->alloc(&h->d_scans, h->n);
    if (!rc) rc = h->alloc(&h->d_hyps, h->n);
    if (rc) return rc;
    HIP_TRY(waitStream(h->stream));
  }
  if (!h->node_readback) HIP_TRY(hipHostMalloc(&h->node_readback, kStagePerFilter * h->n, hipHostMallocDefault));
  // every record type is a multiple of 8 bytes, so each array below is aligned
  char* p = static_cast<char*>(h->node_readback);
  const size_t n = h->n;
  st.odom = reinterpret_cast<navgpu::AmclOdomFilterDev*>(p);
  p += n * sizeof(navgpu::AmclOdomFilterDev);
  st.filters = reinterpret_cast<navgpu::AmclFilterDev*>(p);
  p += n * sizeof(navgpu::AmclFilterDev);
  st.scans = reinterpret_cast<navgpu::AmclScanDev*>(p);
  p += n * sizeof(navgpu::AmclScanDev);
  st.resample = reinterpret_cast<navgpu::AmclResampleFilterDev*>(p);
  p += n * sizeof(navgpu::AmclResampleFilterDev);
  st.hyps = reinterpret_cast<navgpu::AmclHypDev*>(p);
  p += n * sizeof(navgpu::AmclHypDev);
  st.resample_back = reinterpret_cast<navgpu::AmclResampleFilterDev*>(p);
  p += n * sizeof(navgpu::AmclResampleFilterDev);
  st.hyps_back = reinterpret_cast<navgpu::AmclHypDev*>(p);
  return NAVGPU_OK;
}
static_assert(sizeof(navgpu::AmclOdomFilterDev) % 8 == 0 && sizeof(navgpu::AmclFilterDev) % 8 == 0 && sizeof(navgpu::AmclScanDev) % 8 == 0 &&
                  sizeof(navgpu::AmclResampleFilterDev) % 8 == 0 && sizeof(navgpu::AmclHypDev) % 8 == 0,
              "the staging arrays follow each other without padding");
}  // namespace

extern "C" {

int navgpu_amcl_node_configure(navgpu_amcl* h, const navgpu_amcl_node_params* p) {
  if (!h || !p) return NAVGPU_ERR_INVALID;
  const double v[] = {p->d_thresh, p->a_thresh, p->laser_min_range, p->laser_max_range};
  for (double x : v)
    if (x != x) return NAVGPU_ERR_INVALID;
  if (p->resample_interval < 1 || (p->use_odom_integrator != 0 && p->use_odom_integrator != 1)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  h->nparams = *p;
  h->nconfigured = true;
  return NAVGPU_OK;
}

int navgpu_amcl_node_laser_received(navgpu_amcl* h, uint32_t first, uint32_t count, const navgpu_amcl_scan* scans, const float* ranges,
                                    uint64_t seed, navgpu_amcl_node_result* results) {
  if (!h || !scans || !results || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  uint64_t raw_floats = 0;
  for (uint32_t k = 0; k < count; ++k) {
    if (!(scans[k].flags & NAVGPU_AMCL_SCAN_PRESENT)) continue;
    if (scans[k].range_count > (uint32_t)INT32_MAX) {  // AMCLLaserData::range_count is an int
      g_last_error = "navgpu_amcl_node_laser_received: range_count above INT32_MAX";
      return NAVGPU_ERR_INVALID;
    }
    if (scans[k].range_count) raw_floats = std::max<uint64_t>(raw_floats, (uint64_t)scans[k].range_offset + scans[k].range_count);
  }
  if (raw_floats && !ranges) return NAVGPU_ERR_INVALID;
  if (raw_floats > (1ull << 28)) return NAVGPU_ERR_CAPACITY;
  AmclGuard guard_(h);
  if (!h->nconfigured || !h->configured || !h->oconfigured || !h->rconfigured) {
    g_last_error = "navgpu_amcl_node_laser_received before navgpu_amcl_node_configure, navgpu_amcl_laser_configure, "
                   "navgpu_amcl_odom_configure or navgpu_amcl_resample_configure";
    return NAVGPU_ERR_STATE;
  }
  for (uint32_t k = 0; k < count; ++k)
    if ((scans[k].flags & NAVGPU_AMCL_SCAN_PRESENT) && !h->maps[first + k]) {
      g_last_error = "navgpu_amcl_node_laser_received: a filter with a scan has no map";
      return NAVGPU_ERR_STATE;
    }
  const navgpu_amcl_node_params& N = h->nparams;
  const navgpu_amcl_laser_params& P = h->params;
  NodeStage stage{};
  if (int rc = nodeWorkspace(h, stage)) return rc;

  // 1. what the node decides per filter, on a copy of its state (committed after the wait)
  std::vector<navgpu_amcl_node_state> st(count);
  std::vector<NodeDecision> dec(count);
  std::vector<uint8_t> m_moved(count, 0), m_updated(count, 0), m_resampled(count, 0), m_hyp(count, 0);
  std::vector<double> odom((size_t)count * 9, 0.0), range_max(count, 0.0);
  std::vector<uint32_t> range_counts(count, 0);
  std::vector<AmclScanDev> sdev(count, AmclScanDev{});
  bool any_moved = false, any_updated = false, any_resampled = false, any_hyp = false;
  int rc = NAVGPU_OK;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t f = first + k;
    st[k] = h->node[f].s;
    results[k] = navgpu_amcl_node_result{};
    results[k].max_weight_hyp = -1;
    if (!(scans[k].flags & NAVGPU_AMCL_SCAN_PRESENT)) continue;
    NodeDecision& d = dec[k];
    const int rcount = (int)scans[k].range_count;
    if (P.max_beams >= 2 && rcount > 0 && amclBeamStep(P, rcount) < 1) {  // the beam model's loop would never end
      d.refused = true;
      results[k].status = NAVGPU_ERR_INVALID;
      rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_node_laser_received: beam model with 1 <= range_count < max_beams (the reference loops forever)";
      continue;
    }
    d = decide(N, st[k], scans[k].odom_pose);
    std::copy(d.odom, d.odom + 9, &odom[9 * (size_t)k]);
    if (d.updated) {
      convertScan(N, scans[k], sdev[k]);
      range_counts[k] = scans[k].range_count;
      range_max[k] = sdev[k].range_max;
    }
    m_moved[k] = d.moved;
    m_updated[k] = d.updated;
    m_resampled[k] = d.resampled;
    m_hyp[k] = d.resampled || d.force_publication;
    any_moved |= d.moved;
    any_updated |= d.updated;
    any_resampled |= d.resampled;
    any_hyp |= m_hyp[k] != 0;
  }

  // 2. the steps of the slice, back to back
  std::vector<int32_t> tmp(count, 0);
  AmclActionCall ac;
  AmclSensorCall sc;
  AmclResampleCall rcall;
  if (any_updated && P.max_beams >= 2 && raw_floats) {  // first: nothing is in flight yet
    if (raw_floats > h->raw_floats) {
      if (h->d_raw) hipFree(h->d_raw);
      h->d_raw = nullptr;
      h->raw_floats = 0;
      HIP_TRY(hipMalloc(&h->d_raw, sizeof(float) * raw_floats));
      h->raw_floats = raw_floats;
    }
    HIP_TRY(hipMemcpyAsync(h->d_raw, ranges, sizeof(float) * raw_floats, hipMemcpyHostToDevice, h->stream));
  }
  if (any_moved) {
    ac.stage = stage.odom;
    if (int lrc = amclActionEnqueue(h, first, count, odom.data(), true, nullptr, seed, tmp.data(), m_moved.data(), ac)) return lrc;
    amclActionCommit(h, first, count, nullptr, ac);  // the call counters of the filters that moved: the resample draws with the next
  }
  if (any_updated && P.max_beams >= 2) {  // max_beams < 2: AMCLLaser::UpdateSensor returns false (amcl_laser.cpp:163-164)
    sc.scans = &sdev;
    sc.stage = stage.filters;
    sc.scan_stage = stage.scans;
    if (int lrc = amclSensorEnqueue(h, first, count, nullptr, range_counts.data(), range_max.data(), tmp.data(), m_updated.data(), sc))
      return lrc;
  }
  if (any_resampled) {
    rcall.stage = stage.resample;
    if (int lrc = amclResampleEnqueue(h, first, count, true, nullptr, nullptr, nullptr, nullptr, 0, seed, m_resampled.data(), rcall))
      return lrc;
    HIP_TRY(hipMemcpyAsync(stage.resample_back, h->d_rfilters, sizeof(AmclResampleFilterDev) * count, hipMemcpyDeviceToHost, h->stream));
  }
  if (any_hyp) {
    for (uint32_t k = 0; k < count; ++k) {
      AmclHypDev& H = stage.hyps[k];
      H = AmclHypDev{};
      H.active = m_hyp[k];
      H.cluster_count = h->cluster_count[first + k];
      H.from_resample = m_resampled[k];
    }
    HIP_TRY(hipMemcpyAsync(h->d_hyps, stage.hyps, sizeof(AmclHypDev) * count, hipMemcpyHostToDevice, h->stream));
    launch_amcl_hypothesis(h->rs, h->d.max_samples, first, count, h->d_rfilters, h->d_hyps, h->stream);
    if (int lrc = checkLaunch()) return lrc;
    HIP_TRY(hipMemcpyAsync(stage.hyps_back, h->d_hyps, sizeof(AmclHypDev) * count, hipMemcpyDeviceToHost, h->stream));
  }
  if (any_moved || any_updated || any_resampled || any_hyp) HIP_TRY(waitStream(h->stream));

  // 3. the host mirrors, the node state and the results
  if (any_resampled) {
    rcall.fd.assign(stage.resample_back, stage.resample_back + count);
    if (amclResampleCommit(h, first, count, tmp.data(), rcall)) rc = NAVGPU_ERR_INVALID;
  }
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t f = first + k;
    const NodeDecision& d = dec[k];
    navgpu_amcl_node_result& r = results[k];
    if (!(scans[k].flags & NAVGPU_AMCL_SCAN_PRESENT) || d.refused) continue;
    navgpu_amcl_node_state& s = st[k];
    r.moved = d.moved;
    r.updated = d.updated;
    r.resampled = d.resampled;
    r.cloud_due = d.cloud_due;
    r.sample_count = h->sample_count[f];
    r.converged = h->converged[f];
    if (d.resampled) {
      r.status = tmp[k];
      if (h->converged[f] && s.global_localization_active) {  // "Global localization converged!"
        s.global_localization_active = 0;
        r.global_localization_converged = 1;
      }
    }
    if (d.resampled || d.force_publication) {
      fillHypothesis(h, f, stage.hyps_back[k], r);
      if (r.published) {
        // map -> odom = (map -> base) x (odom -> base)^-1 in the plane (amcl_node.cpp:1678-1700 and latest_tf_.inverse() of :1708)
        const double* o = scans[k].odom_pose;
        const double th = r.pose[2] - o[2], c = cos(th), sn = sin(th);
        r.map_to_odom[0] = r.pose[0] - (c * o[0] - sn * o[1]);
        r.map_to_odom[1] = r.pose[1] - (sn * o[0] + c * o[1]);
        r.map_to_odom[2] = th;
        // latest_tf_ = its inverse: {-R(-th) t, -th}
        const double* t = r.map_to_odom;
        s.latest_tf[0] = -(c * t[0] + sn * t[1]);
        s.latest_tf[1] = -(-sn * t[0] + c * t[1]);
        s.latest_tf[2] = -th;
        s.latest_tf_valid = 1;
      }  // else "No pose!"
    } else if (s.latest_tf_valid) {
      r.republish = 1;
      // latest_tf_.inverse() again
      const double th = -s.latest_tf[2], c = cos(th), sn = sin(th);
      r.map_to_odom[0] = -(c * s.latest_tf[0] - sn * s.latest_tf[1]);
      r.map_to_odom[1] = -(sn * s.latest_tf[0] + c * s.latest_tf[1]);
      r.map_to_odom[2] = th;
    }
    h->node[f].s = s;
  }
  return rc;
}

int navgpu_amcl_hypotheses(navgpu_amcl* h, uint32_t first, uint32_t count, navgpu_amcl_node_result* results) {
  if (!h || !results || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  NodeStage stage{};
  if (int rc = nodeWorkspace(h, stage)) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    AmclHypDev& H = stage.hyps[k];
    H = AmclHypDev{};
    H.active = 1;
    H.cluster_count = h->cluster_count[first + k];
  }
  HIP_TRY(hipMemcpyAsync(h->d_hyps, stage.hyps, sizeof(AmclHypDev) * count, hipMemcpyHostToDevice, h->stream));
  launch_amcl_hypothesis(h->rs, h->d.max_samples, first, count, h->d_rfilters, h->d_hyps, h->stream);
  if (int lrc = checkLaunch()) return lrc;
  HIP_TRY(hipMemcpyAsync(stage.hyps_back, h->d_hyps, sizeof(AmclHypDev) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  for (uint32_t k = 0; k < count; ++k) {
    results[k] = navgpu_amcl_node_result{};
    fillHypothesis(h, first + k, stage.hyps_back[k], results[k]);
  }
  return NAVGPU_OK;
}

int navgpu_amcl_node_reset(navgpu_amcl* h, uint32_t first, uint32_t count, int32_t global_localization) {
  if (!h || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_amcl_node_state& s = h->node[first + k].s;
    s.pf_init = 0;
    s.global_localization_active = global_localization ? 1 : 0;
  }
  return NAVGPU_OK;
}

int navgpu_amcl_node_request_nomotion_update(navgpu_amcl* h, uint32_t first, uint32_t count) {
  if (!h || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  for (uint32_t k = 0; k < count; ++k) h->node[first + k].s.force_update = 1;
  return NAVGPU_OK;
}

int navgpu_amcl_node_integrate_odom(navgpu_amcl* h, uint32_t first, uint32_t count, const double* poses) {
  if (!h || !poses || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_amcl_node_state& s = h->node[first + k].s;
    const double* pose = poses + 3 * (size_t)k;
    double* last = s.odom_integrator_last_pose;
    if (!s.odom_integrator_ready) {
      std::fill(s.odom_integrator_absolute_motion, s.odom_integrator_absolute_motion + 3, 0.0);  // resetOdomIntegrator()
      s.odom_integrator_ready = 1;
    } else {
      double delta[3];
      delta[0] = pose[0] - last[0];
      delta[1] = pose[1] - last[1];
      delta[2] = amclAngleDiff(pose[2], last[2]);
      // project bearing change onto average orientation, x is forward translation, y is strafe
      double delta_trans, delta_rot, delta_bearing;
      delta_trans = sqrt(delta[0] * delta[0] + delta[1] * delta[1]);
      delta_rot = delta[2];
      if (delta_trans < 1e-6) {
        // "Assume the very small motion was forward, not strafe."
        delta_bearing = 0;
      } else {
        delta_bearing = amclAngleDiff(atan2(delta[1], delta[0]), last[2] + delta_rot / 2);
      }
      const double cs_bearing = cos(delta_bearing);
      const double sn_bearing = sin(delta_bearing);
      // Accumulate absolute motion
      s.odom_integrator_absolute_motion[0] += fabs(delta_trans * cs_bearing);
      s.odom_integrator_absolute_motion[1] += fabs(delta_trans * sn_bearing);
      s.odom_integrator_absolute_motion[2] += fabs(delta_rot);
    }
    std::copy(pose, pose + 3, last);
  }
  return NAVGPU_OK;
}

int navgpu_amcl_node_get_state(navgpu_amcl* h, uint32_t first, uint32_t count, navgpu_amcl_node_state* states) {
  if (!h || !states || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  for (uint32_t k = 0; k < count; ++k) states[k] = h->node[first + k].s;
  return NAVGPU_OK;
}

int navgpu_amcl_node_set_state(navgpu_amcl* h, uint32_t first, uint32_t count, const navgpu_amcl_node_state* states) {
  if (!h || !states || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_amcl_node_state s = states[k];
    for (int32_t* b : {&s.pf_init, &s.lasers_update, &s.force_update, &s.odom_integrator_ready, &s.global_localization_active,
                       &s.latest_tf_valid})
      *b = *b ? 1 : 0;
    s.reserved = 0;
    h->node[first + k].s = s;
  }
  return NAVGPU_OK;
}

}  // extern "C"
