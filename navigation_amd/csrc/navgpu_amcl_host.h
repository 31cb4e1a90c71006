// Host side of a navgpu_amcl handle, shared by navgpu_amcl.cpp (the steps) and navgpu_amcl_node.cpp (AmclNode's laser cycle).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "navgpu_amcl.h"
#include "navgpu_fleet.h"

namespace navgpu {
// One map_t on the device; several filters may hold the same one (set_map with shared != 0)
struct AmclMap {
  int8_t* occ = nullptr;
  float* dist = nullptr;
  int32_t* free_cells = nullptr;  // occ_state == -1, x-major (AmclNode::free_space_indices, amcl_node.cpp:1028-1033)
  int n_free = 0;
  // the same restricted to map_occ_dist > radius, as the node builds it (init_uniform); rebuilt when the radius or distances change
  int32_t* free_r = nullptr;
  int n_free_r = 0;
  double free_r_radius = 0;
  bool free_r_valid = false;
  int sx = 0, sy = 0;
  double scale = 0, ox = 0, oy = 0, max_occ_dist = 0;
  ~AmclMap() {
    if (occ) hipFree(occ);
    if (dist) hipFree(dist);
    if (free_cells) hipFree(free_cells);
    if (free_r) hipFree(free_r);
  }
};

// What AmclNode keeps between scans for one filter (navgpu_amcl_node_*); the layout is navgpu_amcl_node_state's
struct AmclNodeFilter {
  navgpu_amcl_node_state s{};
  AmclNodeFilter() { s.lasers_update = 1; }  // lasers_update_.push_back(true) (amcl_node.cpp:1344)
};
}  // namespace navgpu

struct navgpu_amcl {
  AmclDev d{};
  uint32_t n = 0;
  int device = 0;
  std::recursive_mutex mu;
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  std::vector<std::shared_ptr<AmclMap>> maps;  // [n]
  std::vector<AmclMapDev> map_desc;            // [n] mirror of d.maps
  std::vector<int32_t> sample_count, converged;
  std::vector<double> laser;                   // [n][3]
  navgpu_amcl_laser_params params{};
  bool configured = false;
  AmclFilterDev* d_filters = nullptr;          // [n]
  double* d_beams = nullptr;                   // [n][2 * max_beams][2] subsampled {range, bearing}
  // resampling (navgpu_amcl_update_resample); the workspace is allocated by the first call
  navgpu_amcl_resample_params rparams{};
  bool rconfigured = false;
  AmclResampleDev rs{};
  bool rs_ready = false;
  AmclResampleFilterDev* d_rfilters = nullptr;  // [n]
  std::vector<int32_t> leaf, cluster_count;     // kd-tree leaf count of the current set at its creation; its cluster count
  std::vector<uint64_t> rng_ctr;                // device draws: calls made per filter
  void* d_upload = nullptr;                     // supplied draws of the last call
  size_t upload_bytes = 0;
  // motion model (navgpu_amcl_update_action); the record workspace is allocated by the first configure
  navgpu_amcl_odom_params oparams{};
  bool oconfigured = false;
  double2* d_records = nullptr;                 // [n][3 max_samples] drand48 Gaussian records {x2, s}
  AmclOdomFilterDev* d_ofilters = nullptr;      // [n]
  AmclInitFilterDev* d_ifilters = nullptr;      // [n] init calls (navgpu_amcl_init_*)
  // AmclNode's laser cycle (navgpu_amcl_node_*, navgpu_amcl_node.cpp); the device records are allocated by the first call
  navgpu_amcl_node_params nparams{};
  bool nconfigured = false;
  std::vector<AmclNodeFilter> node;             // [n]
  AmclScanDev* d_scans = nullptr;               // [n]
  AmclHypDev* d_hyps = nullptr;                 // [n]
  float* d_raw = nullptr;                       // raw LaserScan::ranges of the last call
  size_t raw_floats = 0;
  void* node_readback = nullptr;                // pinned: [n] AmclResampleFilterDev then [n] AmclHypDev
  template <class T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc(&q, bytes) != hipSuccess) {
      g_last_error = "hipMalloc failed (amcl)";
      return NAVGPU_ERR_HIP;
    }
    hipMemsetAsync(q, 0, bytes, stream);
    allocs.push_back(q);
    *p = static_cast<T*>(q);
    return NAVGPU_OK;
  }
  bool rangeOk(uint32_t first, uint32_t count) const { return count > 0 && first < n && count <= n - first; }
  // the resampling workspace (also the init's), allocated by the first call that needs it
  int resampleWorkspace() {
    if (rs_ready) return NAVGPU_OK;
    const size_t ms = d.max_samples, n = this->n;
    AmclResampleDev& r = rs;
    uint32_t P = 1;
    while (P < ms) P <<= 1;
    r.P = P;
    int rc = 0;
#define A(ptr, cnt) \
  if (!rc) rc = alloc(&(ptr), (size_t)(cnt));
    A(r.c, n * (ms + 1));
    A(r.cand, n * ms * 3);
    A(r.cs, n * ms * 2);
    A(r.skey, n * P);
    A(r.sidx, n * P);
    A(r.a, n * P);
    A(r.b, n * P);
    A(r.label, n * ms);
    A(r.ukey, n * ms);
    A(r.cstart, n * ms);
    A(r.cl_count, n * ms);
    A(r.cl_stats, n * ms * 13);
    A(r.set_stats, n * 12);
#undef A
    if (rc) return rc;
    HIP_TRY(waitStream(stream));
    rs_ready = true;
    return NAVGPU_OK;
  }
  int uploadMaps() {
    HIP_TRY(hipMemcpyAsync(d.maps, map_desc.data(), sizeof(AmclMapDev) * n, hipMemcpyHostToDevice, stream));
    HIP_TRY(waitStream(stream));
    return NAVGPU_OK;
  }
};

namespace navgpu {
struct AmclGuard {
  std::lock_guard<std::recursive_mutex> lk;
  explicit AmclGuard(navgpu_amcl* h) : lk(h->mu) { (void)hipSetDevice(h->device); }
};

// amcl_odom.cpp's / amcl_node.cpp's normalize and angle_diff (amcl_odom.cpp:35-56, amcl_node.cpp:87-106: the same text),
// evaluated with the host's libm as the reference evaluates them
inline double amclNormalizeAngle(double z) { return atan2(sin(z), cos(z)); }
inline double amclAngleDiff(double a, double b) {
  a = amclNormalizeAngle(a);
  b = amclNormalizeAngle(b);
  const double d1 = a - b;
  double d2 = 2 * M_PI - fabs(d1);
  if (d1 > 0) d2 *= -1.0;
  if (fabs(d1) < fabs(d2)) return d1;
  return d2;
}

// The three steps as the public calls run them, cut where a caller may want to go on enqueueing: *Enqueue validates nothing
// (the public call has), uploads the per-filter records and launches; the caller waits on the stream; *Commit brings the host
// mirrors up to date.  mask == NULL runs every filter of the slice (the public calls); otherwise filter k runs iff mask[k] != 0,
// through the `active` field of its record, and a skipped filter's status / updated entry is 0.  The handle's lock is held
// by the caller.  A non-zero return is a hard failure (nothing to commit); `soft` is what the public call returns otherwise.
// The per-filter records are uploaded from the call struct, which therefore lives until the caller has waited; a caller that
// must not stall on pageable uploads sets `stage` to pinned memory for `count` records, and they go through it.

// navgpu_amcl_update_action
struct AmclActionCall {
  std::vector<AmclOdomFilterDev> fd;
  bool dev = false;
  int soft = NAVGPU_OK;
  void* stage = nullptr;
};
int amclActionEnqueue(navgpu_amcl* h, uint32_t first, uint32_t count, const double* odom, bool dev, const uint64_t* drand48_state,
                      uint64_t seed, int32_t* status, const uint8_t* mask, AmclActionCall& c);
// device draws: the counters alone, needs no wait; drand48: after the caller has read c.fd back and waited
void amclActionCommit(navgpu_amcl* h, uint32_t first, uint32_t count, uint64_t* drand48_state, const AmclActionCall& c);

// navgpu_amcl_update_sensor.  c.scans == NULL: ranges_xy holds the {range, bearing} pairs (the public call).  Otherwise the beams
// are built on the device by k_amcl_scan from c.scans (one per filter of the slice; step is filled in here) and the raw ranges
// already enqueued into h->d_raw, and the beam-skip state of the filters that run is cleared by that kernel instead of by
// memsets over the slice.
struct AmclSensorCall {
  std::vector<AmclFilterDev> fd;
  std::vector<double> beams;
  std::vector<AmclScanDev>* scans = nullptr;
  int soft = NAVGPU_OK;
  void* stage = nullptr;       // AmclFilterDev records
  void* scan_stage = nullptr;  // AmclScanDev records
};
int amclSensorEnqueue(navgpu_amcl* h, uint32_t first, uint32_t count, const double* ranges_xy, const uint32_t* range_counts,
                      const double* range_max, int32_t* updated, const uint8_t* mask, AmclSensorCall& c);

// navgpu_amcl_update_resample.  The records come back through c.fd, which the caller copies from h->d_rfilters before it waits.
struct AmclResampleCall {
  std::vector<AmclResampleFilterDev> fd;
  bool dev = false;
  void* stage = nullptr;
};

// the source of a record upload: `src` itself, or its copy in pinned `stage`
inline const void* amclStaged(void* stage, const void* src, size_t bytes) {
  if (!stage) return src;
  memcpy(stage, src, bytes);
  return stage;
}
int amclResampleEnqueue(navgpu_amcl* h, uint32_t first, uint32_t count, bool dev, const double* u, const double* systematic_start,
                        const double* random_poses, const uint32_t* random_pose_counts, uint64_t pool_total, uint64_t seed,
                        const uint8_t* mask, AmclResampleCall& c);
int amclResampleCommit(navgpu_amcl* h, uint32_t first, uint32_t count, int32_t* status, const AmclResampleCall& c);

// The models' subsampling step of a scan (amcl_laser.cpp:265, 334-338, 417-421, 637-641); < 1 where the beam model's loop would
// never end.  max_beams >= 2.
int amclBeamStep(const navgpu_amcl_laser_params& P, int rcount);
}  // namespace navgpu
