// navgpu_amcl_*: host side of the amcl laser update for a batch of particle filters (see amcl_kernels.hip and include/navgpu.h).
#include "navgpu_amcl_host.h"

#include <array>

namespace {
bool isFinite(double v) { return std::isfinite(v); }

bool paramsValid(const navgpu_amcl_laser_params& p) {
  if (p.model_type < NAVGPU_AMCL_MODEL_BEAM || p.model_type > NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_GOMPERTZ) return false;
  if (p.max_beams < 0 || (p.do_beamskip != 0 && p.do_beamskip != 1)) return false;
  const double v[] = {p.z_hit, p.z_short, p.z_max, p.z_rand, p.sigma_hit, p.lambda_short, p.chi_outlier, p.beam_skip_distance,
                      p.beam_skip_threshold, p.beam_skip_error_threshold, p.gompertz_a, p.gompertz_b, p.gompertz_c, p.input_shift,
                      p.input_scale, p.output_shift, p.off_map_factor, p.non_free_space_factor, p.non_free_space_radius, p.alpha_slow,
                      p.alpha_fast};
  for (double x : v)
    if (x != x) return false;
  return true;
}
}  // namespace

extern "C" {

int navgpu_amcl_create(uint32_t n_filters, uint32_t max_samples, uint32_t max_beams, int32_t device, navgpu_amcl** out) {
  if (!out || !n_filters || !max_samples || !max_beams) return NAVGPU_ERR_INVALID;
  // filters sit on a grid dimension of the launches (<= 65535); sample indices and counts are int32
  if (max_beams > (uint32_t)kAmclMaxBeams || n_filters > (uint32_t)kAmclMaxFilters || max_samples > (uint32_t)INT32_MAX ||
      (uint64_t)n_filters * max_samples > (1ull << 28))
    return NAVGPU_ERR_CAPACITY;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    g_last_error = "no usable HIP device (navgpu has no CPU fallback)";
    return NAVGPU_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  navgpu_amcl* h = new navgpu_amcl();
  h->n = n_filters;
  h->device = device;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    g_last_error = "hipStreamCreate failed";
    return NAVGPU_ERR_HIP;
  }
  h->maps.resize(n_filters);
  h->map_desc.assign(n_filters, AmclMapDev{});
  h->sample_count.assign(n_filters, 0);
  h->converged.assign(n_filters, 0);
  h->laser.assign((size_t)n_filters * 3, 0.0);
  h->leaf.assign(n_filters, 0);
  h->cluster_count.assign(n_filters, 0);
  h->rng_ctr.assign(n_filters, 0);
  h->node.assign(n_filters, AmclNodeFilter{});
  AmclDev& d = h->d;
  d.max_samples = max_samples;
  d.max_beams = max_beams;
  int rc = 0;
#define A(ptr, cnt) \
  if (!rc) rc = h->alloc(&(ptr), (size_t)(cnt));
  A(d.poses, (size_t)n_filters * max_samples * 3);
  A(d.weights, (size_t)n_filters * max_samples);
  A(d.w, (size_t)n_filters * 2);
  A(d.maps, n_filters);
  A(d.obs_count, (size_t)n_filters * max_beams);
  A(d.obs_mask, (size_t)n_filters * max_beams);
  A(d.skip_info, (size_t)n_filters * 2);
  A(h->d_filters, n_filters);
  A(h->d_beams, (size_t)n_filters * 2 * max_beams * 2);
  A(h->d_rfilters, n_filters);
#undef A
  if (!rc && waitStream(h->stream) != hipSuccess) rc = NAVGPU_ERR_HIP;
  if (rc) {
    navgpu_amcl_destroy(h);
    return rc;
  }
  *out = h;
  return NAVGPU_OK;
}

int navgpu_amcl_destroy(navgpu_amcl* h) {
  if (!h) return NAVGPU_ERR_INVALID;
  (void)hipSetDevice(h->device);
  if (h->stream) waitStream(h->stream);
  h->maps.clear();
  for (void* p : h->allocs) hipFree(p);
  if (h->d_upload) hipFree(h->d_upload);
  if (h->d_raw) hipFree(h->d_raw);
  if (h->node_readback) hipHostFree(h->node_readback);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return NAVGPU_OK;
}

}  // extern "C"

namespace {
// The free-cell list of a map for random poses: cells with occ_state == -1 in AmclNode's x-major order (amcl_node.cpp:1028-1033,
// with its default laser_non_free_space_radius 0 every free cell passes map_occ_dist > radius)
int freeCells(AmclMap& m, hipStream_t s) {
  std::vector<int8_t> occ((size_t)m.sx * m.sy);
  HIP_TRY(hipMemcpyAsync(occ.data(), m.occ, occ.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(waitStream(s));
  std::vector<int32_t> list;
  for (int i = 0; i < m.sx; ++i)
    for (int j = 0; j < m.sy; ++j)
      if (occ[i + (size_t)j * m.sx] == -1) list.push_back(i + j * m.sx);
  m.n_free = (int)list.size();
  if (list.empty()) return NAVGPU_OK;
  HIP_TRY(hipMalloc(&m.free_cells, list.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpyAsync(m.free_cells, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(waitStream(s));
  return NAVGPU_OK;
}

// pf_kdtree_insert's leaf count (pf_kdtree.c:110-120): distinct floor(pose / {0.5, 0.5, 10 deg}) keys of a set, as pf_init_model
// leaves it.  Non-finite bins all count as one key.
int32_t leafCount(const double* poses, int n) {
  std::vector<std::array<double, 3>> keys((size_t)n);
  const double size[3] = {0.50, 0.50, (10 * M_PI / 180)};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const double b = std::floor(poses[3 * (size_t)i + a] / size[a]);
      keys[i][a] = std::isfinite(b) ? b : INFINITY;
    }
  std::sort(keys.begin(), keys.end());
  return (int32_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
}

int beamStep(const navgpu_amcl_laser_params& P, int rcount) { return navgpu::amclBeamStep(P, rcount); }

// Maps of a slice: `src` is OccupancyGrid data (height x width, scaled up by `factor` on the device) or, with `cells`, map_t
// occ_state values copied as they are (factor 1); scale and the centre origin (ox, oy) are map_t's own.
int setMaps(navgpu_amcl* h, uint32_t first, uint32_t count, const int8_t* src, uint32_t width, uint32_t height, int factor, bool cells,
            double scale, double ox, double oy, int32_t shared, double max_occ_dist) {
  const uint64_t sx = (uint64_t)width * factor, sy = (uint64_t)height * factor;
  AmclGuard guard_(h);
  // map_update_cspace: CachedDistanceMap::cell_radius_ = max_dist / scale, an int
  const double rd = max_occ_dist / scale;
  const int radius = rd >= 2147483647.0 ? 2147483647 : (int)rd;
  const size_t msg_cells = (size_t)width * height, cells_n = (size_t)(sx * sy);
  int8_t* d_msg = nullptr;
  int32_t* d_g = nullptr;
  HIP_TRY(hipMalloc(&d_msg, msg_cells));
  if (hipMalloc(&d_g, cells_n * sizeof(int32_t)) != hipSuccess) {
    hipFree(d_msg);
    g_last_error = "hipMalloc failed (amcl map)";
    return NAVGPU_ERR_HIP;
  }
  int rc = NAVGPU_OK;
  std::vector<std::shared_ptr<AmclMap>> made;
  const uint32_t n_maps = shared ? 1u : count;
  for (uint32_t k = 0; k < n_maps && !rc; ++k) {
    auto m = std::make_shared<AmclMap>();
    m->sx = (int)sx;
    m->sy = (int)sy;
    m->scale = scale;
    m->ox = ox;
    m->oy = oy;
    m->max_occ_dist = max_occ_dist;
    if (hipMalloc(&m->occ, cells_n) != hipSuccess || hipMalloc(&m->dist, cells_n * sizeof(float)) != hipSuccess) {
      g_last_error = "hipMalloc failed (amcl map)";
      rc = NAVGPU_ERR_HIP;
      break;
    }
    if (hipMemcpyAsync(cells ? m->occ : d_msg, src + k * msg_cells, msg_cells, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
      rc = NAVGPU_ERR_HIP;
      break;
    }
    if (!cells) launch_amcl_convert(d_msg, width, height, factor, m->occ, m->sx, m->sy, h->stream);
    launch_amcl_cspace(m->occ, m->sx, m->sy, radius, scale, max_occ_dist, d_g, m->dist, h->stream);
    if (!rc) rc = checkLaunch();
    if (waitStream(h->stream) != hipSuccess) rc = NAVGPU_ERR_HIP;  // the staging buffers are reused by the next map
    if (!rc) rc = freeCells(*m, h->stream);
    made.push_back(m);
  }
  hipFree(d_msg);
  hipFree(d_g);
  if (rc) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    const auto& m = made[shared ? 0 : k];
    h->maps[first + k] = m;
    h->map_desc[first + k] = AmclMapDev{m->occ, m->dist, m->free_cells, m->n_free, m->sx, m->sy, m->scale, m->ox, m->oy, m->max_occ_dist};
  }
  return h->uploadMaps();
}

void odomConstants(const navgpu_amcl_odom_params& P, const double* o, double* k);
}  // namespace

// The steps' bodies (navgpu_amcl_host.h): what the public calls below run, and what navgpu_amcl_node_laser_received chains
namespace navgpu {

int amclBeamStep(const navgpu_amcl_laser_params& P, int rcount) {
  int step;
  if (P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB) {
    step = (int)ceil(rcount / static_cast<double>(P.max_beams));
    if (step < 1) step = 1;
  } else {
    step = (rcount - 1) / (P.max_beams - 1);
    if (step < 1 && P.model_type != NAVGPU_AMCL_MODEL_BEAM) step = 1;
  }
  return step;
}

int amclSensorEnqueue(navgpu_amcl* h, uint32_t first, uint32_t count, const double* ranges_xy, const uint32_t* range_counts,
                      const double* range_max, int32_t* updated, const uint8_t* mask, AmclSensorCall& c) {
  const navgpu_amcl_laser_params& P = h->params;
  // Subsample every filter's scan with the model's step (amcl_laser.cpp:265, 334-338, 417-421, 637-641)
  std::vector<AmclFilterDev>& fd = c.fd;
  std::vector<double>& beams = c.beams;
  std::vector<AmclScanDev>* const scans = c.scans;
  fd.assign(count, AmclFilterDev{});
  beams.clear();
  if (!scans) beams.reserve((size_t)count * 4 * P.max_beams);
  int rc = NAVGPU_OK, max_samples = 0, max_nb = 0;
  const double* src = ranges_xy;
  size_t n_pairs = 0;
  bool any = false;
  for (uint32_t k = 0; k < count; ++k) {
    const int rcount = (int)range_counts[k];
    const uint32_t f = first + k;
    AmclFilterDev& e = fd[k];
    e = AmclFilterDev{};
    if (mask && !mask[k]) {  // e.active == 0
      updated[k] = 0;
      if (scans) (*scans)[k].active = 0;
      if (!scans) src += 2 * (size_t)rcount;
      continue;
    }
    const int step = amclBeamStep(P, rcount);
    e.sample_count = h->sample_count[f];
    e.converged = h->converged[f];
    e.range_max = range_max[k];
    std::copy(&h->laser[3 * (size_t)f], &h->laser[3 * (size_t)f] + 3, e.laser);
    e.beam_off = (uint32_t)n_pairs;
    e.active = 1;
    if (step < 1 && rcount > 0) {  // the beam model's loop would never end
      e.active = 0;
      updated[k] = NAVGPU_ERR_INVALID;
      rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_update_sensor: beam model with 1 <= range_count < max_beams (the reference loops forever)";
      if (scans) (*scans)[k].active = 0;
    } else {
      updated[k] = 1;
      any = true;
      if (scans) {
        (*scans)[k].active = 1;
        (*scans)[k].step = step;
        if (rcount > 0) n_pairs += ((size_t)rcount + step - 1) / step;
      } else {
        for (int i = 0; i < rcount; i += step) {
          beams.push_back(src[2 * (size_t)i]);
          beams.push_back(src[2 * (size_t)i + 1]);
        }
        n_pairs = beams.size() / 2;
      }
      e.n_beams = (int)(n_pairs - e.beam_off);
      max_samples = std::max(max_samples, e.sample_count);
      max_nb = std::max(max_nb, e.n_beams);
    }
    if (!scans) src += 2 * (size_t)rcount;
  }
  c.soft = rc;
  if (2 * n_pairs > (size_t)h->n * 2 * h->d.max_beams * 2) return NAVGPU_ERR_CAPACITY;  // cannot happen: < 2 max_beams per filter
  if (mask && !any) return NAVGPU_OK;
  if (!beams.empty())
    HIP_TRY(hipMemcpyAsync(h->d_beams, beams.data(), sizeof(double) * beams.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_filters, amclStaged(c.stage, fd.data(), sizeof(AmclFilterDev) * count), sizeof(AmclFilterDev) * count,
                         hipMemcpyHostToDevice, h->stream));
  if (scans) {
    HIP_TRY(hipMemcpyAsync(h->d_scans, amclStaged(c.scan_stage, scans->data(), sizeof(AmclScanDev) * count), sizeof(AmclScanDev) * count,
                           hipMemcpyHostToDevice, h->stream));
    launch_amcl_scan(h->d, first, count, h->d_filters, h->d_scans, h->d_raw, h->d_beams, h->stream);
  } else {
    HIP_TRY(hipMemsetAsync(h->d.obs_count + (size_t)first * h->d.max_beams, 0, sizeof(int32_t) * count * h->d.max_beams, h->stream));
    HIP_TRY(hipMemsetAsync(h->d.obs_mask + (size_t)first * h->d.max_beams, 0, (size_t)count * h->d.max_beams, h->stream));
    HIP_TRY(hipMemsetAsync(h->d.skip_info + 2 * (size_t)first, 0, sizeof(int32_t) * 2 * count, h->stream));
  }
  if (P.model_type == NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB && P.do_beamskip)
    launch_amcl_laser(h->d, P, first, count, h->d_filters, h->d_beams, max_samples, max_nb, 1, h->stream);
  launch_amcl_laser(h->d, P, first, count, h->d_filters, h->d_beams, max_samples, max_nb, 0, h->stream);
  launch_amcl_normalize(h->d, P, first, count, h->d_filters, h->stream);
  return checkLaunch();
}

int amclResampleEnqueue(navgpu_amcl* h, uint32_t first, uint32_t count, bool dev, const double* u, const double* systematic_start,
                        const double* random_poses, const uint32_t* random_pose_counts, uint64_t pool_total, uint64_t seed,
                        const uint8_t* mask, AmclResampleCall& c) {
  const navgpu_amcl_resample_params& R = h->rparams;
  const bool sys = R.resample_model == NAVGPU_AMCL_RESAMPLE_SYSTEMATIC;
  const size_t ms = h->d.max_samples;
  AmclResampleDev& r = h->rs;
  if (int rc = h->resampleWorkspace()) return rc;
  // supplied draws: {u_flag, u_pick} pairs (multinomial) then the random-pose pool, in one upload
  const size_t u_doubles = (!dev && !sys) ? (size_t)count * ms * 2 : 0, bytes = sizeof(double) * (u_doubles + 3 * pool_total);
  r.u = nullptr;
  r.pool = nullptr;
  if (bytes) {
    if (bytes > h->upload_bytes) {
      if (h->d_upload) hipFree(h->d_upload);
      h->d_upload = nullptr;
      h->upload_bytes = 0;
      HIP_TRY(hipMalloc(&h->d_upload, bytes));
      h->upload_bytes = bytes;
    }
    double* up = static_cast<double*>(h->d_upload);
    if (u_doubles) HIP_TRY(hipMemcpyAsync(up, u, sizeof(double) * u_doubles, hipMemcpyHostToDevice, h->stream));
    if (pool_total)
      HIP_TRY(hipMemcpyAsync(up + u_doubles, random_poses, sizeof(double) * 3 * pool_total, hipMemcpyHostToDevice, h->stream));
    r.u = up;
    r.pool = up + u_doubles;
  }
  c.dev = dev;
  std::vector<AmclResampleFilterDev>& fd = c.fd;
  fd.assign(count, AmclResampleFilterDev{});
  uint64_t pool_off = 0;
  for (uint32_t k = 0; k < count; ++k) {
    AmclResampleFilterDev& e = fd[k];
    const uint32_t f = first + k;
    e.sample_count = h->sample_count[f];
    e.leaf_in = h->leaf[f];
    e.pool_count = dev ? 0 : (int32_t)random_pose_counts[k];
    e.pool_off = pool_off;
    pool_off += dev ? 0 : random_pose_counts[k];
    e.rng_ctr = h->rng_ctr[f];
    e.sys_start = (!dev && sys) ? systematic_start[k] : 0.0;
    e.active = (mask && !mask[k]) ? 0 : 1;
    e.status = NAVGPU_ERR_INVALID;
  }
  HIP_TRY(hipMemcpyAsync(h->d_rfilters, amclStaged(c.stage, fd.data(), sizeof(AmclResampleFilterDev) * count),
                         sizeof(AmclResampleFilterDev) * count, hipMemcpyHostToDevice, h->stream));
  const AmclResampleParamsDev P{R.resample_model, R.min_samples, (int32_t)ms, dev ? 1 : 0, R.pop_err, R.pop_z, R.dist_threshold, seed};
  launch_amcl_resample(h->d, r, P, first, count, h->d_rfilters, h->stream);
  return checkLaunch();
}

int amclResampleCommit(navgpu_amcl* h, uint32_t first, uint32_t count, int32_t* status, const AmclResampleCall& c) {
  int rc = NAVGPU_OK;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t f = first + k;
    const AmclResampleFilterDev& e = c.fd[k];
    if (!e.active) {
      status[k] = 0;
      continue;
    }
    status[k] = e.status;
    if (c.dev) ++h->rng_ctr[f];
    if (e.status != NAVGPU_OK) {
      rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_update_resample: a filter has no samples, too few supplied random poses, no free cell or a pose "
                     "outside the histogram's range";
      continue;
    }
    h->sample_count[f] = e.count;
    h->leaf[f] = e.leaf_out;
    h->converged[f] = e.converged;
    h->cluster_count[f] = e.cluster_count;
  }
  return rc;
}

int amclActionEnqueue(navgpu_amcl* h, uint32_t first, uint32_t count, const double* odom, bool dev, const uint64_t* drand48_state,
                      uint64_t seed, int32_t* status, const uint8_t* mask, AmclActionCall& c) {
  std::vector<AmclOdomFilterDev>& fd = c.fd;
  fd.assign(count, AmclOdomFilterDev{});
  c.dev = dev;
  int rc = NAVGPU_OK, max_count = 0;
  for (uint32_t k = 0; k < count; ++k) {
    AmclOdomFilterDev& e = fd[k];
    const uint32_t f = first + k;
    status[k] = NAVGPU_OK;
    if (mask && !mask[k]) continue;  // e.active == 0
    e.sample_count = h->sample_count[f];
    e.active = 1;
    e.state = dev ? 0 : drand48_state[k];
    e.rng_ctr = h->rng_ctr[f];
    odomConstants(h->oparams, odom + 9 * (size_t)k, e.k);
    if (!dev && drand48_state[k] > kAmclDrand48Mask) {
      e.active = 0;
      status[k] = NAVGPU_ERR_INVALID;
      rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_update_action: a drand48 state >= 2^48";
      continue;
    }
    max_count = std::max(max_count, e.sample_count);
  }
  c.soft = rc;
  HIP_TRY(hipMemcpyAsync(h->d_ofilters, amclStaged(c.stage, fd.data(), sizeof(AmclOdomFilterDev) * count),
                         sizeof(AmclOdomFilterDev) * count, hipMemcpyHostToDevice, h->stream));
  if (!dev) launch_amcl_drand48_gauss(h->d_records, h->d.max_samples, count, h->d_ofilters, h->stream);
  launch_amcl_odom(h->d, h->oparams.model_type, dev ? 1 : 0, seed, h->d_records, first, count, max_count, h->d_ofilters, h->stream);
  return checkLaunch();
}

void amclActionCommit(navgpu_amcl* h, uint32_t first, uint32_t count, uint64_t* drand48_state, const AmclActionCall& c) {
  for (uint32_t k = 0; k < count; ++k) {
    if (!c.fd[k].active) continue;
    if (c.dev)
      ++h->rng_ctr[first + k];
    else
      drand48_state[k] = c.fd[k].state;
  }
}

}  // namespace navgpu

extern "C" {

int navgpu_amcl_set_map(navgpu_amcl* h, uint32_t first, uint32_t count, const int8_t* occupancy, uint32_t width, uint32_t height,
                        double resolution, const double* origin_xy, int32_t scale_up_factor, int32_t shared, double max_occ_dist) {
  if (!h || !occupancy || !origin_xy || !h->rangeOk(first, count) || !width || !height || !(resolution > 0) || !isFinite(resolution) ||
      scale_up_factor < 1 || scale_up_factor > 16 || !(max_occ_dist >= 0) || !isFinite(max_occ_dist) || !isFinite(origin_xy[0]) ||
      !isFinite(origin_xy[1]))
    return NAVGPU_ERR_INVALID;
  const uint64_t sx = (uint64_t)width * scale_up_factor, sy = (uint64_t)height * scale_up_factor;
  if (sx > (uint64_t)kAmclMaxMapSide || sy > (uint64_t)kAmclMaxMapSide) return NAVGPU_ERR_CAPACITY;
  // AmclNode::convertMap: size = msg size * f, scale = resolution / f, origin moved to the map centre
  const double scale = resolution / scale_up_factor;
  const double ox = origin_xy[0] + (int)(sx / 2) * scale, oy = origin_xy[1] + (int)(sy / 2) * scale;
  return setMaps(h, first, count, occupancy, width, height, scale_up_factor, false, scale, ox, oy, shared, max_occ_dist);
}

int navgpu_amcl_set_map_cells(navgpu_amcl* h, uint32_t first, uint32_t count, const int8_t* occ_state, uint32_t size_x, uint32_t size_y,
                              double scale, double origin_x, double origin_y, int32_t shared, double max_occ_dist) {
  if (!h || !occ_state || !h->rangeOk(first, count) || !size_x || !size_y || !(scale > 0) || !isFinite(scale) || !(max_occ_dist >= 0) ||
      !isFinite(max_occ_dist) || !isFinite(origin_x) || !isFinite(origin_y))
    return NAVGPU_ERR_INVALID;
  if (size_x > (uint32_t)kAmclMaxMapSide || size_y > (uint32_t)kAmclMaxMapSide) return NAVGPU_ERR_CAPACITY;
  return setMaps(h, first, count, occ_state, size_x, size_y, 1, true, scale, origin_x, origin_y, shared, max_occ_dist);
}

int navgpu_amcl_set_distance_map(navgpu_amcl* h, uint32_t first, uint32_t count, const float* distances, int32_t shared) {
  if (!h || !distances || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  for (uint32_t k = 0; k < count; ++k)
    if (!h->maps[first + k]) {
      g_last_error = "navgpu_amcl_set_distance_map: filter without a map";
      return NAVGPU_ERR_STATE;
    }
  if (shared)
    for (uint32_t k = 1; k < count; ++k)
      if (h->maps[first + k]->sx != h->maps[first]->sx || h->maps[first + k]->sy != h->maps[first]->sy) return NAVGPU_ERR_INVALID;
  size_t off = 0;
  for (uint32_t k = 0; k < count; ++k) {
    const AmclMap& m = *h->maps[first + k];
    const size_t cells = (size_t)m.sx * m.sy;
    HIP_TRY(hipMemcpyAsync(m.dist, distances + off, cells * sizeof(float), hipMemcpyHostToDevice, h->stream));
    h->maps[first + k]->free_r_valid = false;
    if (!shared) off += cells;
  }
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_amcl_distance_map(navgpu_amcl* h, uint32_t filter, float* out) {
  if (!h || !out || filter >= h->n) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  const auto& m = h->maps[filter];
  if (!m) return NAVGPU_ERR_STATE;
  HIP_TRY(hipMemcpyAsync(out, m->dist, (size_t)m->sx * m->sy * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_amcl_laser_configure(navgpu_amcl* h, const navgpu_amcl_laser_params* p) {
  if (!h || !p || !paramsValid(*p)) return NAVGPU_ERR_INVALID;
  if ((uint32_t)p->max_beams > h->d.max_beams) return NAVGPU_ERR_CAPACITY;
  AmclGuard guard_(h);
  h->params = *p;
  h->configured = true;
  return NAVGPU_OK;
}

int navgpu_amcl_set_laser_pose(navgpu_amcl* h, uint32_t first, uint32_t count, const double* xyth) {
  if (!h || !xyth || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  std::copy(xyth, xyth + 3 * (size_t)count, h->laser.begin() + 3 * (size_t)first);
  return NAVGPU_OK;
}

int navgpu_amcl_set_samples(navgpu_amcl* h, uint32_t first, uint32_t count, const int32_t* sample_counts, const double* poses,
                            const double* weights, const int32_t* converged) {
  if (!h || !sample_counts || !poses || !weights || !converged || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k) {
    if (sample_counts[k] < 0) return NAVGPU_ERR_INVALID;
    if ((uint32_t)sample_counts[k] > h->d.max_samples) return NAVGPU_ERR_CAPACITY;
  }
  AmclGuard guard_(h);
  const size_t ms = h->d.max_samples;
  HIP_TRY(hipMemcpyAsync(h->d.poses + first * ms * 3, poses, sizeof(double) * count * ms * 3, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d.weights + first * ms, weights, sizeof(double) * count * ms, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));
  for (uint32_t k = 0; k < count; ++k) {
    h->sample_count[first + k] = sample_counts[k];
    h->converged[first + k] = converged[k] ? 1 : 0;
    h->leaf[first + k] = leafCount(poses + (size_t)k * ms * 3, sample_counts[k]);
  }
  return NAVGPU_OK;
}

int navgpu_amcl_get_samples(navgpu_amcl* h, uint32_t first, uint32_t count, int32_t* sample_counts, double* poses, double* weights,
                            int32_t* converged) {
  if (!h || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  const size_t ms = h->d.max_samples;
  if (poses) HIP_TRY(hipMemcpyAsync(poses, h->d.poses + first * ms * 3, sizeof(double) * count * ms * 3, hipMemcpyDeviceToHost, h->stream));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, h->d.weights + first * ms, sizeof(double) * count * ms, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  for (uint32_t k = 0; k < count; ++k) {
    if (sample_counts) sample_counts[k] = h->sample_count[first + k];
    if (converged) converged[k] = h->converged[first + k];
  }
  return NAVGPU_OK;
}

int navgpu_amcl_set_filter_state(navgpu_amcl* h, uint32_t first, uint32_t count, const double* w) {
  if (!h || !w || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  HIP_TRY(hipMemcpyAsync(h->d.w + 2 * (size_t)first, w, sizeof(double) * 2 * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_amcl_get_filter_state(navgpu_amcl* h, uint32_t first, uint32_t count, double* w) {
  if (!h || !w || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  HIP_TRY(hipMemcpyAsync(w, h->d.w + 2 * (size_t)first, sizeof(double) * 2 * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_amcl_update_sensor(navgpu_amcl* h, uint32_t first, uint32_t count, const double* ranges_xy, const uint32_t* range_counts,
                              const double* range_max, int32_t* updated) {
  if (!h || !range_counts || !range_max || !updated || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  if (!h->configured) {
    g_last_error = "navgpu_amcl_update_sensor before navgpu_amcl_laser_configure";
    return NAVGPU_ERR_STATE;
  }
  const navgpu_amcl_laser_params& P = h->params;
  uint64_t total_ranges = 0;
  for (uint32_t k = 0; k < count; ++k) {
    if (range_counts[k] > (uint32_t)INT32_MAX) {  // AMCLLaserData::range_count is an int
      g_last_error = "navgpu_amcl_update_sensor: range_count above INT32_MAX";
      return NAVGPU_ERR_INVALID;
    }
    total_ranges += range_counts[k];
  }
  if (total_ranges && !ranges_xy) return NAVGPU_ERR_INVALID;
  if (P.max_beams < 2) {  // AMCLLaser::UpdateSensor returns false (amcl_laser.cpp:163-164)
    std::fill(updated, updated + count, 0);
    return NAVGPU_OK;
  }
  for (uint32_t k = 0; k < count; ++k) {  // every map carries its distance map (set_map computes it), so a map is all it needs
    if (!h->maps[first + k]) {
      g_last_error = "navgpu_amcl_update_sensor: a filter has no map";
      return NAVGPU_ERR_STATE;
    }
  }
  AmclSensorCall c;
  const int lrc = amclSensorEnqueue(h, first, count, ranges_xy, range_counts, range_max, updated, nullptr, c);
  if (lrc == NAVGPU_ERR_CAPACITY) return lrc;
  HIP_TRY(waitStream(h->stream));
  return lrc ? lrc : c.soft;
}

int navgpu_amcl_beam_skip_state(navgpu_amcl* h, uint32_t filter, int32_t* obs_count, uint8_t* obs_mask, int32_t* error, int32_t* active) {
  if (!h || filter >= h->n) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  const size_t mb = h->d.max_beams;
  int32_t info[2];
  HIP_TRY(hipMemcpyAsync(info, h->d.skip_info + 2 * (size_t)filter, sizeof(info), hipMemcpyDeviceToHost, h->stream));
  if (obs_count) HIP_TRY(hipMemcpyAsync(obs_count, h->d.obs_count + filter * mb, sizeof(int32_t) * mb, hipMemcpyDeviceToHost, h->stream));
  if (obs_mask) HIP_TRY(hipMemcpyAsync(obs_mask, h->d.obs_mask + filter * mb, mb, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  if (active) *active = info[0];
  if (error) *error = info[1];
  return NAVGPU_OK;
}

int navgpu_amcl_resample_configure(navgpu_amcl* h, const navgpu_amcl_resample_params* p) {
  if (!h || !p) return NAVGPU_ERR_INVALID;
  if ((p->resample_model != NAVGPU_AMCL_RESAMPLE_MULTINOMIAL && p->resample_model != NAVGPU_AMCL_RESAMPLE_SYSTEMATIC) ||
      p->min_samples < 0 || (uint32_t)p->min_samples > h->d.max_samples || !(p->pop_err > 0) || !isFinite(p->pop_err) ||
      !isFinite(p->pop_z) || p->dist_threshold != p->dist_threshold)
    return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  h->rparams = *p;
  h->rconfigured = true;
  return NAVGPU_OK;
}

int navgpu_amcl_set_kd_leaf_counts(navgpu_amcl* h, uint32_t first, uint32_t count, const int32_t* leaf_counts) {
  if (!h || !leaf_counts || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k)
    if (leaf_counts[k] < 0) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  std::copy(leaf_counts, leaf_counts + count, h->leaf.begin() + first);
  return NAVGPU_OK;
}

int navgpu_amcl_get_kd_leaf_counts(navgpu_amcl* h, uint32_t first, uint32_t count, int32_t* leaf_counts) {
  if (!h || !leaf_counts || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  std::copy(h->leaf.begin() + first, h->leaf.begin() + first + count, leaf_counts);
  return NAVGPU_OK;
}

int navgpu_amcl_set_rng_counters(navgpu_amcl* h, uint32_t first, uint32_t count, const uint64_t* counters) {
  if (!h || !counters || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  std::copy(counters, counters + count, h->rng_ctr.begin() + first);
  return NAVGPU_OK;
}

int navgpu_amcl_get_rng_counters(navgpu_amcl* h, uint32_t first, uint32_t count, uint64_t* counters) {
  if (!h || !counters || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  std::copy(h->rng_ctr.begin() + first, h->rng_ctr.begin() + first + count, counters);
  return NAVGPU_OK;
}

int navgpu_amcl_update_resample(navgpu_amcl* h, uint32_t first, uint32_t count, int32_t draw_source, const double* u,
                                const double* systematic_start, const double* random_poses, const uint32_t* random_pose_counts, uint64_t seed,
                                int32_t* status) {
  if (!h || !status || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  if (draw_source != NAVGPU_AMCL_DRAW_SUPPLIED && draw_source != NAVGPU_AMCL_DRAW_DEVICE) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  if (!h->rconfigured) {
    g_last_error = "navgpu_amcl_update_resample before navgpu_amcl_resample_configure";
    return NAVGPU_ERR_STATE;
  }
  const bool sys = h->rparams.resample_model == NAVGPU_AMCL_RESAMPLE_SYSTEMATIC, dev = draw_source == NAVGPU_AMCL_DRAW_DEVICE;
  uint64_t pool_total = 0;
  if (!dev) {
    if (!random_pose_counts || (!sys && !u) || (sys && !systematic_start)) return NAVGPU_ERR_INVALID;
    for (uint32_t k = 0; k < count; ++k) pool_total += random_pose_counts[k];
    if (pool_total && !random_poses) return NAVGPU_ERR_INVALID;
    if (pool_total > (uint64_t)INT32_MAX) return NAVGPU_ERR_CAPACITY;
  } else {
    for (uint32_t k = 0; k < count; ++k)
      if (!h->maps[first + k]) {
        g_last_error = "navgpu_amcl_update_resample: device draws for a filter without a map";
        return NAVGPU_ERR_STATE;
      }
  }
  AmclResampleCall c;
  if (int lrc = amclResampleEnqueue(h, first, count, dev, u, systematic_start, random_poses, random_pose_counts, pool_total, seed, nullptr, c))
    return lrc;
  HIP_TRY(hipMemcpyAsync(c.fd.data(), h->d_rfilters, sizeof(AmclResampleFilterDev) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return amclResampleCommit(h, first, count, status, c);
}

int navgpu_amcl_get_clusters(navgpu_amcl* h, uint32_t filter, int32_t* cluster_count, uint32_t capacity, int32_t* counts, double* weights,
                             double* means, double* covs, double* set_mean, double* set_cov) {
  if (!h || !cluster_count || filter >= h->n) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  const int32_t C = h->cluster_count[filter];
  *cluster_count = C;
  if (!h->rs_ready || C == 0) {
    g_last_error = "navgpu_amcl_get_clusters: the filter has not been resampled";
    return NAVGPU_ERR_STATE;
  }
  const size_t ms = h->d.max_samples, fo = (size_t)filter * ms, nc = std::min<size_t>((size_t)C, capacity);
  std::vector<int32_t> cnt(nc);
  std::vector<double> st(nc * 13), ss(12);
  if (nc) {
    HIP_TRY(hipMemcpyAsync(cnt.data(), h->rs.cl_count + fo, sizeof(int32_t) * nc, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(st.data(), h->rs.cl_stats + fo * 13, sizeof(double) * nc * 13, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipMemcpyAsync(ss.data(), h->rs.set_stats + 12 * (size_t)filter, sizeof(double) * 12, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  for (size_t k = 0; k < nc; ++k) {
    if (counts) counts[k] = cnt[k];
    if (weights) weights[k] = st[13 * k];
    if (means) std::copy(&st[13 * k + 1], &st[13 * k + 4], means + 3 * k);
    if (covs) std::copy(&st[13 * k + 4], &st[13 * k + 13], covs + 9 * k);
  }
  if (set_mean) std::copy(ss.begin(), ss.begin() + 3, set_mean);
  if (set_cov) std::copy(ss.begin() + 3, ss.end(), set_cov);
  return (size_t)C > capacity ? NAVGPU_ERR_CAPACITY : NAVGPU_OK;
}

}  // extern "C"

namespace {
// amcl_odom.cpp's normalize / angle_diff (:35-56): navgpu_amcl_host.h
double normalizeAngle(double z) { return amclNormalizeAngle(z); }
double angleDiff(double a, double b) { return amclAngleDiff(a, b); }

// What AMCLOdom::UpdateAction computes from the odometry alone (amcl_odom.cpp:128-379), in its own expressions; the per-particle
// part is k_amcl_odom.  The diff models evaluate their stddevs inside the sample loop: the same value for every sample.
void odomConstants(const navgpu_amcl_odom_params& P, const double* o, double* k) {
  const double* pose = o;
  const double* delta = o + 3;
  const double* absm = o + 6;
  const double old_theta = pose[2] - delta[2];  // pf_vector_sub(ndata->pose, ndata->delta).v[2]
  const double a1 = P.alpha1, a2 = P.alpha2, a3 = P.alpha3, a4 = P.alpha4, a5 = P.alpha5;
  std::fill(k, k + kAmclOdomConsts, 0.0);
  switch (P.model_type) {
    case NAVGPU_AMCL_ODOM_OMNI:
    case NAVGPU_AMCL_ODOM_OMNI_CORRECTED: {
      const double delta_trans = sqrt(delta[0] * delta[0] + delta[1] * delta[1]);
      const double delta_rot = delta[2];
      double trans_sd = (a3 * (delta_trans * delta_trans) + a1 * (delta_rot * delta_rot));
      double rot_sd = (a4 * (delta_rot * delta_rot) + a2 * (delta_trans * delta_trans));
      double strafe_sd = (a1 * (delta_rot * delta_rot) + a5 * (delta_trans * delta_trans));
      if (P.model_type == NAVGPU_AMCL_ODOM_OMNI_CORRECTED) {
        trans_sd = sqrt(trans_sd);
        rot_sd = sqrt(rot_sd);
        strafe_sd = sqrt(strafe_sd);
      }
      k[0] = angleDiff(atan2(delta[1], delta[0]), old_theta);
      k[1] = delta_trans;
      k[2] = delta_rot;
      k[3] = trans_sd;
      k[4] = rot_sd;
      k[5] = strafe_sd;
      break;
    }
    case NAVGPU_AMCL_ODOM_DIFF:
    case NAVGPU_AMCL_ODOM_DIFF_CORRECTED: {
      double delta_rot1;
      if (sqrt(delta[1] * delta[1] + delta[0] * delta[0]) < 0.01)
        delta_rot1 = 0.0;
      else
        delta_rot1 = angleDiff(atan2(delta[1], delta[0]), old_theta);
      const double delta_trans = sqrt(delta[0] * delta[0] + delta[1] * delta[1]);
      const double delta_rot2 = angleDiff(delta[2], delta_rot1);
      const double n1 = std::min(fabs(angleDiff(delta_rot1, 0.0)), fabs(angleDiff(delta_rot1, M_PI)));
      const double n2 = std::min(fabs(angleDiff(delta_rot2, 0.0)), fabs(angleDiff(delta_rot2, M_PI)));
      double rot1_sd = a1 * n1 * n1 + a2 * delta_trans * delta_trans;
      double trans_sd = a3 * delta_trans * delta_trans + a4 * n1 * n1 + a4 * n2 * n2;
      double rot2_sd = a1 * n2 * n2 + a2 * delta_trans * delta_trans;
      if (P.model_type == NAVGPU_AMCL_ODOM_DIFF_CORRECTED) {
        rot1_sd = sqrt(rot1_sd);
        trans_sd = sqrt(trans_sd);
        rot2_sd = sqrt(rot2_sd);
      }
      k[0] = normalizeAngle(delta_rot1);  // angle_diff(delta_rot1, .)'s first step, the same for every sample
      k[1] = normalizeAngle(delta_rot2);
      k[2] = delta_trans;
      k[3] = rot1_sd;
      k[4] = trans_sd;
      k[5] = rot2_sd;
      break;
    }
    default: {  // NAVGPU_AMCL_ODOM_GAUSSIAN
      const double delta_trans = sqrt(delta[0] * delta[0] + delta[1] * delta[1]);
      const double delta_rot = delta[2];
      const double t2 = absm[0] * absm[0], s2 = absm[1] * absm[1], r2 = absm[2] * absm[2];
      k[0] = angleDiff(atan2(delta[1], delta[0]), old_theta);
      k[1] = delta_trans;
      k[2] = delta_rot;
      k[3] = delta[2] / 2;
      k[4] = sqrt(a3 * t2 + a4 * r2);  // trans
      k[5] = sqrt(a4 * r2 + a5 * s2);  // strafe
      k[6] = sqrt(a1 * r2 + a2 * t2);  // rot
      break;
    }
  }
}
}  // namespace

extern "C" {

int navgpu_amcl_odom_configure(navgpu_amcl* h, const navgpu_amcl_odom_params* p) {
  if (!h || !p) return NAVGPU_ERR_INVALID;
  if (p->model_type < NAVGPU_AMCL_ODOM_DIFF || p->model_type > NAVGPU_AMCL_ODOM_GAUSSIAN) return NAVGPU_ERR_INVALID;
  const double v[] = {p->alpha1, p->alpha2, p->alpha3, p->alpha4, p->alpha5};
  for (double x : v)
    if (x != x) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  if (!h->d_records) {
    int rc = 0;
    if (!rc) rc = h->alloc(&h->d_records, (size_t)h->n * 3 * h->d.max_samples);
    if (!rc) rc = h->alloc(&h->d_ofilters, h->n);
    if (rc) return rc;
    HIP_TRY(waitStream(h->stream));
  }
  h->oparams = *p;
  h->oconfigured = true;
  return NAVGPU_OK;
}

int navgpu_amcl_update_action(navgpu_amcl* h, uint32_t first, uint32_t count, const double* odom, int32_t draw_source,
                              uint64_t* drand48_state, uint64_t seed, int32_t* status) {
  if (!h || !status || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  if (draw_source != NAVGPU_AMCL_DRAW_DRAND48 && draw_source != NAVGPU_AMCL_DRAW_DEVICE) return NAVGPU_ERR_INVALID;
  const bool dev = draw_source == NAVGPU_AMCL_DRAW_DEVICE;
  if (!odom || (!dev && !drand48_state)) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  if (!h->oconfigured) {
    g_last_error = "navgpu_amcl_update_action before navgpu_amcl_odom_configure";
    return NAVGPU_ERR_STATE;
  }
  AmclActionCall c;
  if (int lrc = amclActionEnqueue(h, first, count, odom, dev, drand48_state, seed, status, nullptr, c)) return lrc;
  if (!dev) HIP_TRY(hipMemcpyAsync(c.fd.data(), h->d_ofilters, sizeof(AmclOdomFilterDev) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  amclActionCommit(h, first, count, drand48_state, c);
  return c.soft;
}

}  // extern "C"

namespace {
// pf_matrix_unitary (pf_vector.c:222-276): the eigen-decomposition of a symmetric 3 x 3 matrix by Householder reduction to
// tridiagonal form, then the implicit-shift QL iteration, eigenvalues ascending (the EISPACK tred2 / tql2 pair as JAMA states
// it).  Every operation keeps the order of that formulation, so the host's IEEE fp64 (no contraction) reproduces the
// reference's rotation and eigenvalues bit for bit.  false when the iteration does not settle (a non-finite matrix).
bool symmetricEigen3(const double a[9], double vec[3][3], double val[3]) {
  double* const dg = val;  // the diagonal as the reduction and the iteration go on
  double off[3];           // the sub-diagonal
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) vec[r][c] = a[3 * r + c];
  for (int c = 0; c < 3; ++c) dg[c] = vec[2][c];
  // 1. Householder: row `row` of the remaining block is folded onto the sub-diagonal, rows 2 then 1
  for (int row = 2; row >= 1; --row) {
    double norm1 = 0.0, hh = 0.0;
    for (int k = 0; k < row; ++k) norm1 = norm1 + fabs(dg[k]);
    if (norm1 == 0.0) {
      off[row] = dg[row - 1];
      for (int c = 0; c < row; ++c) {
        dg[c] = vec[row - 1][c];
        vec[row][c] = 0.0;
        vec[c][row] = 0.0;
      }
      dg[row] = hh;
      continue;
    }
    for (int k = 0; k < row; ++k) {
      dg[k] /= norm1;
      hh += dg[k] * dg[k];
    }
    double lead = dg[row - 1], root = sqrt(hh);
    if (lead > 0) root = -root;
    off[row] = norm1 * root;
    hh = hh - lead * root;
    dg[row - 1] = lead - root;
    for (int c = 0; c < row; ++c) off[c] = 0.0;
    for (int c = 0; c < row; ++c) {
      const double u = dg[c];
      vec[c][row] = u;
      double acc = off[c] + vec[c][c] * u;
      for (int k = c + 1; k <= row - 1; ++k) {
        acc += vec[k][c] * dg[k];
        off[k] += vec[k][c] * u;
      }
      off[c] = acc;
    }
    double dot = 0.0;
    for (int c = 0; c < row; ++c) {
      off[c] /= hh;
      dot += off[c] * dg[c];
    }
    const double half = dot / (hh + hh);
    for (int c = 0; c < row; ++c) off[c] -= half * dg[c];
    for (int c = 0; c < row; ++c) {
      const double u = dg[c], q = off[c];
      for (int k = c; k <= row - 1; ++k) vec[k][c] -= (u * off[k] + q * dg[k]);
      dg[c] = vec[row - 1][c];
      vec[row][c] = 0.0;
    }
    dg[row] = hh;
  }
  // 2. the accumulated transformation
  for (int c = 0; c < 2; ++c) {
    vec[2][c] = vec[c][c];
    vec[c][c] = 1.0;
    const double hh = dg[c + 1];
    if (hh != 0.0) {
      for (int k = 0; k <= c; ++k) dg[k] = vec[k][c + 1] / hh;
      for (int j = 0; j <= c; ++j) {
        double acc = 0.0;
        for (int k = 0; k <= c; ++k) acc += vec[k][c + 1] * vec[k][j];
        for (int k = 0; k <= c; ++k) vec[k][j] -= acc * dg[k];
      }
    }
    for (int k = 0; k <= c; ++k) vec[k][c + 1] = 0.0;
  }
  for (int c = 0; c < 3; ++c) {
    dg[c] = vec[2][c];
    vec[2][c] = 0.0;
  }
  vec[2][2] = 1.0;
  off[0] = 0.0;
  // 3. QL with implicit shifts on the tridiagonal (dg, off)
  off[0] = off[1];
  off[1] = off[2];
  off[2] = 0.0;
  double shift = 0.0, bound = 0.0;
  const double eps = 0x1p-52;
  for (int l = 0; l < 3; ++l) {
    const double here = fabs(dg[l]) + fabs(off[l]);
    bound = bound > here ? bound : here;
    int m = l;
    while (m < 2 && !(fabs(off[m]) <= eps * bound)) ++m;  // off[2] == 0 always stops the search
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 64) return false;
        const double g0 = dg[l];
        double p = (dg[l + 1] - g0) / (2.0 * off[l]);
        double r = sqrt(p * p + 1.0 * 1.0);
        if (p < 0) r = -r;
        dg[l] = off[l] / (p + r);
        dg[l + 1] = off[l] * (p + r);
        const double next = dg[l + 1];
        double h = g0 - dg[l];
        for (int i = l + 2; i < 3; ++i) dg[i] -= h;
        shift = shift + h;
        p = dg[m];
        double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
        const double el1 = off[l + 1];
        for (int i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          const double g = c * off[i];
          h = c * p;
          r = sqrt(p * p + off[i] * off[i]);
          off[i + 1] = s * r;
          s = off[i] / r;
          c = p / r;
          p = c * dg[i] - s * g;
          dg[i + 1] = h + s * (c * g + s * dg[i]);
          for (int k = 0; k < 3; ++k) {
            const double v1 = vec[k][i + 1];
            vec[k][i + 1] = s * vec[k][i] + c * v1;
            vec[k][i] = c * vec[k][i] - s * v1;
          }
        }
        p = -s * s2 * c3 * el1 * off[l] / next;
        off[l] = s * p;
        dg[l] = c * p;
      } while (fabs(off[l]) > eps * bound);
    }
    dg[l] = dg[l] + shift;
    off[l] = 0.0;
  }
  // 4. ascending order, columns with them (selection of the smallest, as the reference)
  for (int i = 0; i < 2; ++i) {
    int k = i;
    double p = dg[i];
    for (int j = i + 1; j < 3; ++j)
      if (dg[j] < p) {
        k = j;
        p = dg[j];
      }
    if (k != i) {
      dg[k] = dg[i];
      dg[i] = p;
      for (int j = 0; j < 3; ++j) std::swap(vec[j][i], vec[j][k]);
    }
  }
  return true;
}

// 48-bit LCG state advanced k steps (drand48's a = 0x5DEECE66D, c = 0xB)
uint64_t drand48Advance(uint64_t x, uint64_t k) {
  uint64_t a = 1, c = 0, ba = 0x5DEECE66Dull, bc = 0xB;
  while (k) {
    if (k & 1) {
      a = (ba * a) & kAmclDrand48Mask;
      c = (ba * c + bc) & kAmclDrand48Mask;
    }
    bc = (ba * bc + bc) & kAmclDrand48Mask;
    ba = (ba * ba) & kAmclDrand48Mask;
    k >>= 1;
  }
  return (a * x + c) & kAmclDrand48Mask;
}

constexpr uint64_t kInitDefaultCandidatesPerSample = 100;  // max_candidates = 0: 100 x max_samples per filter

// The free cells of map m with map_occ_dist > radius (amcl_node.cpp:1026-1033), kept on the map until the radius or its
// distances change
int freeCellsBeyond(AmclMap& m, double radius, hipStream_t s) {
  if (m.free_r_valid && m.free_r_radius == radius) return NAVGPU_OK;
  const size_t cells = (size_t)m.sx * m.sy;
  std::vector<int8_t> occ(cells);
  std::vector<float> dist(cells);
  HIP_TRY(hipMemcpyAsync(occ.data(), m.occ, cells, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(dist.data(), m.dist, cells * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(waitStream(s));
  std::vector<int32_t> list;
  for (int i = 0; i < m.sx; ++i)
    for (int j = 0; j < m.sy; ++j) {
      const size_t c = i + (size_t)j * m.sx;
      if (occ[c] == -1 && (double)dist[c] > radius) list.push_back((int32_t)c);
    }
  if (m.free_r) hipFree(m.free_r);
  m.free_r = nullptr;
  m.n_free_r = (int)list.size();
  m.free_r_valid = false;
  if (!list.empty()) {
    HIP_TRY(hipMalloc(&m.free_r, list.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(m.free_r, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(waitStream(s));
  }
  m.free_r_radius = radius;
  m.free_r_valid = true;
  return NAVGPU_OK;
}

// Launch an init over the slice and commit what succeeded: the set is max_samples poses of weight 1 / max_samples, w_slow =
// w_fast = 0, unconverged, with its leaf count and clusters
int runInit(navgpu_amcl* h, uint32_t first, uint32_t count, const AmclInitParamsDev& p, std::vector<AmclInitFilterDev>& fd,
            const std::vector<double>& beams, int max_nb) {
  if (int rc = h->resampleWorkspace()) return rc;
  if (p.gaussian && !p.draw_device && !h->d_records) {
    if (int rc = h->alloc(&h->d_records, (size_t)h->n * 3 * h->d.max_samples)) return rc;
  }
  if (!h->d_ifilters) {
    if (int rc = h->alloc(&h->d_ifilters, h->n)) return rc;
  }
  if (!beams.empty())
    HIP_TRY(hipMemcpyAsync(h->d_beams, beams.data(), sizeof(double) * beams.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_ifilters, fd.data(), sizeof(AmclInitFilterDev) * count, hipMemcpyHostToDevice, h->stream));
  launch_amcl_init(h->d, h->rs, p, h->params, h->d_beams, max_nb, h->d_records, first, count, h->d_ifilters, h->stream);
  const int lrc = checkLaunch();
  if (lrc) return lrc;
  HIP_TRY(hipMemcpyAsync(fd.data(), h->d_ifilters, sizeof(AmclInitFilterDev) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t f = first + k;
    if (!fd[k].active || fd[k].status != NAVGPU_OK) continue;
    h->sample_count[f] = (int32_t)h->d.max_samples;
    h->converged[f] = 0;
    h->leaf[f] = fd[k].leaf_out;
    h->cluster_count[f] = fd[k].cluster_count;
  }
  return NAVGPU_OK;
}
}  // namespace

extern "C" {

int navgpu_amcl_init_gaussian(navgpu_amcl* h, uint32_t first, uint32_t count, const double* mean, const double* cov, int32_t draw_source,
                              uint64_t* drand48_state, uint64_t seed, int32_t* status) {
  if (!h || !status || !mean || !cov || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  if (draw_source != NAVGPU_AMCL_DRAW_DRAND48 && draw_source != NAVGPU_AMCL_DRAW_DEVICE) return NAVGPU_ERR_INVALID;
  const bool dev = draw_source == NAVGPU_AMCL_DRAW_DEVICE;
  if (!dev && !drand48_state) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  std::vector<AmclInitFilterDev> fd(count);
  int rc = NAVGPU_OK;
  for (uint32_t k = 0; k < count; ++k) {
    AmclInitFilterDev& e = fd[k];
    e = AmclInitFilterDev{};
    e.active = 1;
    e.status = NAVGPU_OK;
    e.state = dev ? 0 : drand48_state[k];
    e.rng_ctr = h->rng_ctr[first + k];
    status[k] = NAVGPU_OK;
    double vec[3][3], val[3];
    bool ok = dev || drand48_state[k] <= kAmclDrand48Mask;
    for (int a = 0; a < 3; ++a) ok = ok && isFinite(mean[3 * (size_t)k + a]);
    for (int a = 0; a < 9; ++a) ok = ok && isFinite(cov[9 * (size_t)k + a]);
    ok = ok && symmetricEigen3(cov + 9 * (size_t)k, vec, val);
    if (!ok) {
      e.active = 0;
      status[k] = NAVGPU_ERR_INVALID;
      rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_init_gaussian: a drand48 state >= 2^48 or a non-finite mean or covariance";
      continue;
    }
    for (int a = 0; a < 3; ++a) {
      e.mean[a] = mean[3 * (size_t)k + a];
      e.cd[a] = sqrt(val[a]);  // pf_pdf_gaussian_alloc (pf_pdf.c:60-62); NaN for a negative eigenvalue
      for (int b = 0; b < 3; ++b) e.cr[3 * a + b] = vec[a][b];
    }
  }
  AmclInitParamsDev p{};
  p.gaussian = 1;
  p.draw_device = dev ? 1 : 0;
  p.seed = seed;
  const int irc = runInit(h, first, count, p, fd, {}, 0);
  if (irc) return irc;
  for (uint32_t k = 0; k < count; ++k) {
    if (!fd[k].active) continue;
    if (dev) ++h->rng_ctr[first + k];
    if (fd[k].status != NAVGPU_OK) {
      status[k] = fd[k].status;
      rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_init_gaussian: a non-finite pose or a pose outside the histogram's range";
    } else if (!dev) {
      drand48_state[k] = fd[k].state;
    }
  }
  return rc;
}

int navgpu_amcl_init_uniform(navgpu_amcl* h, uint32_t first, uint32_t count, const navgpu_amcl_uniform_params* params, const double* ranges_xy,
                             const uint32_t* range_counts, const double* range_max, int32_t draw_source, uint64_t* drand48_state,
                             uint64_t seed, uint64_t* candidates_used, int32_t* status) {
  if (!h || !params || !status || !h->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  if (draw_source != NAVGPU_AMCL_DRAW_DRAND48 && draw_source != NAVGPU_AMCL_DRAW_DEVICE) return NAVGPU_ERR_INVALID;
  const bool dev = draw_source == NAVGPU_AMCL_DRAW_DEVICE;
  if (!dev && !drand48_state) return NAVGPU_ERR_INVALID;
  const bool scan = ranges_xy || range_counts;  // both NULL: no scan yet (last_laser_data_ == NULL)
  if (scan && (!range_counts || !range_max)) return NAVGPU_ERR_INVALID;
  const double thr = params->starting_weight_threshold, mult = params->deweight_multiplier;
  if (thr != thr || mult != mult) return NAVGPU_ERR_INVALID;
  AmclGuard guard_(h);
  const size_t ms = h->d.max_samples;
  const uint64_t cap = params->max_candidates ? params->max_candidates
                                              : std::min<uint64_t>(kInitDefaultCandidatesPerSample * ms, dev ? (1ull << 32) : (1ull << 40));
  if (cap > (1ull << 40) || (dev && cap > (1ull << 32))) return NAVGPU_ERR_INVALID;  // device retries are numbered in 32 bits
  for (uint32_t k = 0; k < count; ++k)
    if (!h->maps[first + k]) {
      g_last_error = "navgpu_amcl_init_uniform: a filter has no map";
      return NAVGPU_ERR_STATE;
    }
  if (scan && !h->configured) {
    g_last_error = "navgpu_amcl_init_uniform: a scan before navgpu_amcl_laser_configure";
    return NAVGPU_ERR_STATE;
  }
  const navgpu_amcl_laser_params& P = h->params;
  const bool scored = scan && thr > 0.0 && mult < 1.0 && mult >= 0.0;  // amcl_node.cpp:1253
  const double radius = h->configured ? P.non_free_space_radius : 0.0;
  std::vector<AmclInitFilterDev> fd(count);
  std::vector<double> beams;
  int rc = NAVGPU_OK, max_nb = 0;
  const double* src = ranges_xy;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t f = first + k;
    AmclInitFilterDev& e = fd[k];
    e = AmclInitFilterDev{};
    e.active = 1;
    e.status = NAVGPU_OK;
    e.state = dev ? 0 : drand48_state[k];
    e.rng_ctr = h->rng_ctr[f];
    status[k] = NAVGPU_OK;
    AmclMap& m = *h->maps[f];
    if (int frc = freeCellsBeyond(m, radius, h->stream)) return frc;
    e.free_cells = m.free_r;
    e.n_free = m.n_free_r;
    const int rcount = scan ? (int)std::min<uint32_t>(range_counts[k], (uint32_t)INT32_MAX) : 0;
    if (scan && range_counts[k] > (uint32_t)INT32_MAX) return NAVGPU_ERR_INVALID;
    if (scored) {
      if (rcount && !ranges_xy) return NAVGPU_ERR_INVALID;
      std::copy(&h->laser[3 * (size_t)f], &h->laser[3 * (size_t)f] + 3, e.laser);
      e.range_max = range_max[k];
      e.beam_off = (uint32_t)(beams.size() / 2);
      const int step = P.max_beams < 2 ? 1 : beamStep(P, rcount);
      if (step < 1 && rcount > 0) {
        e.active = 0;
        status[k] = NAVGPU_ERR_INVALID;
        if (rc != NAVGPU_ERR_CAPACITY) rc = NAVGPU_ERR_INVALID;
        g_last_error = "navgpu_amcl_init_uniform: beam model with 1 <= range_count < max_beams (the reference loops forever)";
      } else if (P.max_beams >= 2) {
        for (int i = 0; i < rcount; i += step) {
          beams.push_back(src[2 * (size_t)i]);
          beams.push_back(src[2 * (size_t)i + 1]);
        }
      }
      e.n_beams = (int)(beams.size() / 2 - e.beam_off);
      max_nb = std::max(max_nb, e.n_beams);
      src += 2 * (size_t)rcount;
    }
    if (e.active && (e.n_free <= 0 || (!dev && drand48_state[k] > kAmclDrand48Mask))) {
      e.active = 0;
      status[k] = NAVGPU_ERR_INVALID;
      if (rc != NAVGPU_ERR_CAPACITY) rc = NAVGPU_ERR_INVALID;
      g_last_error = "navgpu_amcl_init_uniform: a map without free cells or a drand48 state >= 2^48";
    }
    if (e.active && !scored && cap < ms) {
      e.active = 0;
      status[k] = NAVGPU_ERR_CAPACITY;
      rc = NAVGPU_ERR_CAPACITY;
    }
  }
  if (beams.size() > (size_t)h->n * 2 * h->d.max_beams * 2) return NAVGPU_ERR_CAPACITY;  // cannot happen: < 2 max_beams per filter
  AmclInitParamsDev p{};
  p.draw_device = dev ? 1 : 0;
  p.scored = scored ? 1 : 0;
  p.threshold = thr;
  p.multiplier = mult;
  p.max_candidates = cap;
  p.seed = seed;
  const int irc = runInit(h, first, count, p, fd, beams, max_nb);
  if (irc) return irc;
  for (uint32_t k = 0; k < count; ++k) {
    if (!fd[k].active) {
      if (candidates_used) candidates_used[k] = 0;
      continue;
    }
    const uint64_t used = scored ? fd[k].used : ms;
    if (candidates_used) candidates_used[k] = used;
    if (dev) ++h->rng_ctr[first + k];
    if (fd[k].status != NAVGPU_OK) {
      status[k] = fd[k].status;
      if (rc == NAVGPU_OK || fd[k].status == NAVGPU_ERR_CAPACITY) rc = fd[k].status;
      g_last_error = "navgpu_amcl_init_uniform: a filter needed more than max_candidates candidates, or a pose outside the histogram";
    } else if (!dev) {
      drand48_state[k] = drand48Advance(drand48_state[k], 2 * used);
    }
  }
  return rc;
}

}  // extern "C"
