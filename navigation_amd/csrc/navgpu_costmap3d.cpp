// navgpu_costmap3d_*: host side of the batched Costmap3DQuery (costmap3d_kernels.hip, include/navgpu.h).
// Every argument check runs before the device is opened (openDevice) and before anything is queued.
#include <cfloat>
#include <cmath>
#include <map>
#include <memory>
#include <type_traits>

#include "navgpu_costmap3d.h"
#include "navgpu_fleet.h"

// what navgpu_costmap3d_configure_layers adds to a handle (include/navgpu_costmap3d_layers.h)
struct C3dLayers {
  std::vector<navgpu_c3d_layer> layers;
  std::vector<uint32_t> index;     // per layer: its slot (costmap layers) or its number among the cylinder layers
  uint32_t n_cyl = 0, max_points = 0;
  C3dLayersDev ly{};
  std::vector<uint32_t> cur;       // [n][nc] which plane set is current
  std::vector<uint32_t> full;      // [n] size_changed_ / copy_full_map_
  std::vector<uint8_t> moved;      // [n] the window moved since the last update (navgpu_costmap3d_roll): its 2-D bounds are the window
  struct Cyl { bool has = false; double x = 0, y = 0; };
  std::vector<Cyl> prev;           // [n][n_cyl] CylinderClearingLayer3D::clearing_bounds_map_, as the position it was built round
  std::vector<void*> allocs;
  uint8_t *d_stage = nullptr, *h_stage = nullptr;  // a call's records: one upload (h_stage pinned); the read-back comes into its tail
  size_t stage_bytes = 0;
  float* d_points = nullptr;       // [max_points][4]
  int8_t* d_grid = nullptr;        // a static grid on its way in; grows on demand
  size_t grid_bytes = 0;
  bool resident = false;           // the device buffers exist (openLayers)
};

// what navgpu_costmap3d_publisher_configure, _export and _layer_update_cells add to a handle (include/navgpu_costmap3d_publish.h)
struct C3dPublish {
  bool enabled = false;             // publisher_configure: the three vectors below exist
  std::vector<uint32_t> seq;        // [n] Costmap3DPublisher::update_seq_
  std::vector<int64_t> window;      // [n][3] the lattice origin a shadow was taken at
  std::vector<uint8_t> has_window;  // [n]
  uint64_t* d_shadow = nullptr;     // [n][shadow_planes][cols] the master as last published; comes with the first DELTA
  uint32_t shadow_planes = 0;
  struct Sub { bool first_full = false, using_updates = false; uint32_t n_updates = 0, last_seq = 0; };
  std::vector<Sub> subs;            // [n][nc] OctomapServerLayer3D's subscription state; sized by the first update_cells after a configure_layers
  const void* subs_of = nullptr;    // the C3dLayers the states belong to
  // a call's device blocks, grown on demand
  uint8_t *d_stage = nullptr, *h_stage = nullptr;  // records up, counts down (h_stage pinned)
  size_t stage_bytes = 0;
  uint32_t* d_counts = nullptr;     // counts, offsets, totals
  size_t count_words = 0;
  navgpu_c3d_leaf *d_values = nullptr, *d_bounds = nullptr;
  size_t value_capacity = 0, bounds_capacity = 0;
  uint64_t* d_scratch = nullptr;    // [scratch_msgs][4][cols]; all zero between calls
  uint32_t* d_touched = nullptr;    // [scratch_msgs][tw]
  size_t scratch_msgs = 0;
};

struct navgpu_costmap3d {
  navgpu_costmap3d_desc desc{};
  C3dLayers* layered = nullptr;
  C3dPublish* pub = nullptr;
  C3dDev dv{};
  bool opened = false;
  std::recursive_mutex mu;  // calls on one handle are serialised inside the library (as on a fleet)
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  std::vector<double> origins;          // [n][3] host copy
  C3dBoxCells* d_boxes = nullptr;       // [max_boxes]
  C3dBoxCells* h_boxes = nullptr;       // pinned: a set_boxes call's records until its copy has run
  uint8_t *d_in = nullptr, *d_out = nullptr;  // a query call's upload and read-back
  uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned
  uint8_t *d_roll = nullptr, *h_roll = nullptr;  // a roll's or a reset_bounding_box call's records (h_roll pinned); come with the first such call
  bool have_mesh = false;
  template <class T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc(&q, bytes) != hipSuccess) {
      g_last_error = "hipMalloc failed (costmap3d)";
      return NAVGPU_ERR_HIP;
    }
    hipMemsetAsync(q, 0, bytes, stream);
    allocs.push_back(q);
    *p = static_cast<T*>(q);
    return NAVGPU_OK;
  }
};

namespace {

struct C3dGuard {
  std::lock_guard<std::recursive_mutex> lk;
  explicit C3dGuard(navgpu_costmap3d* h) : lk(h->mu) {}
};

constexpr size_t kInBytesPerPose = 7 * sizeof(double) + sizeof(int32_t) + sizeof(navgpu_c3d_run) + 2;
constexpr size_t kOutBytesPerPose = sizeof(double) + sizeof(navgpu_c3d_run_result);

// the first call that needs the device: the stream and every buffer, all or nothing
int openDevice(navgpu_costmap3d* h) {
  if (h->opened) {
    HIP_TRY(hipSetDevice(h->desc.device));
    return NAVGPU_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || h->desc.device >= ndev) {
    g_last_error = "no usable HIP device (navgpu has no CPU fallback)";
    return NAVGPU_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(h->desc.device));
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    h->stream = nullptr;
    g_last_error = "hipStreamCreate failed";
    return NAVGPU_ERR_HIP;
  }
  const navgpu_costmap3d_desc& ds = h->desc;
  C3dDev& dv = h->dv;
  int rc = h->alloc(&dv.planes, (size_t)ds.n_instances * 2 * dv.cols);
  if (!rc) rc = h->alloc(&dv.origins, (size_t)ds.n_instances * 3);
  if (!rc) rc = h->alloc(&dv.verts, (size_t)ds.max_triangles * 9);
  if (!rc) rc = h->alloc(&h->d_boxes, ds.max_boxes);
  if (!rc) rc = h->alloc(&h->d_in, kInBytesPerPose * ds.max_poses);
  if (!rc) rc = h->alloc(&h->d_out, kOutBytesPerPose * ds.max_poses);
  auto pinned = [&](auto** p, size_t bytes) {
    if (!rc && hipHostMalloc((void**)p, std::max<size_t>(bytes, 16), hipHostMallocDefault) != hipSuccess) {
      *p = nullptr;
      g_last_error = "hipHostMalloc failed (costmap3d)";
      rc = NAVGPU_ERR_HIP;
    }
  };
  pinned(&h->h_boxes, sizeof(C3dBoxCells) * ds.max_boxes);
  pinned(&h->h_in, kInBytesPerPose * ds.max_poses);
  pinned(&h->h_out, kOutBytesPerPose * ds.max_poses);
  if (!rc && hipMemcpyAsync(dv.origins, h->origins.data(), sizeof(double) * h->origins.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = NAVGPU_ERR_HIP;
  if (!rc && waitStream(h->stream) != hipSuccess) rc = NAVGPU_ERR_HIP;
  if (rc) {  // the next call starts over
    for (void* p : h->allocs) hipFree(p);
    h->allocs.clear();
    for (void* p : {(void*)h->h_boxes, (void*)h->h_in, (void*)h->h_out})
      if (p) hipHostFree(p);
    h->h_boxes = nullptr;
    h->h_in = h->h_out = nullptr;
    hipStreamDestroy(h->stream);
    h->stream = nullptr;
    return rc;
  }
  h->opened = true;
  return NAVGPU_OK;
}

bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// a box's cell range along one axis: its lower face in cells from the origin, an integer to 1e-6 of a cell
bool alignedCell(double centre, double size, double origin, double res, int64_t* first) {
  const double f = (centre - 0.5 * size - origin) / res;
  if (!std::isfinite(f) || std::fabs(f) > 1073741824.0) return false;
  const double r = std::nearbyint(f);
  if (std::fabs(f - r) > 1e-6) return false;
  *first = (int64_t)r;
  return true;
}

// what a query call checks, packs and runs; poses7 indexed by the runs
int runQuery(navgpu_costmap3d* h, uint32_t n_runs, const navgpu_c3d_run* runs, const double* poses7, int32_t mode, const uint8_t* regions,
             const uint8_t* obstacles, const double* region_scale, double distance_limit, int32_t lazy, double* pose_costs_out,
             navgpu_c3d_run_result* results_out) {
  const navgpu_costmap3d_desc& ds = h->desc;
  if (mode != NAVGPU_C3D_COST && mode != NAVGPU_C3D_COLLISION_ONLY && mode != NAVGPU_C3D_DISTANCE) {
    g_last_error = "navgpu_costmap3d_query: mode must be COST, COLLISION_ONLY or DISTANCE (no signed distance)";
    return NAVGPU_ERR_INVALID;
  }
  if (std::isnan(distance_limit)) return NAVGPU_ERR_INVALID;
  if (n_runs && (!runs || !poses7)) return NAVGPU_ERR_INVALID;
  if (n_runs > ds.max_poses) return NAVGPU_ERR_CAPACITY;
  uint64_t n_poses = 0;
  for (uint32_t r = 0; r < n_runs; ++r) {
    if (runs[r].instance >= ds.n_instances) return NAVGPU_ERR_INVALID;
    n_poses = std::max<uint64_t>(n_poses, (uint64_t)runs[r].first_pose + runs[r].n_poses);
  }
  if (n_poses > ds.max_poses) return NAVGPU_ERR_CAPACITY;
  std::vector<int32_t> pose_inst((size_t)n_poses, -1);
  bool prism = false;
  for (uint32_t r = 0; r < n_runs; ++r)
    for (uint32_t j = 0; j < runs[r].n_poses; ++j) {
      const size_t p = (size_t)runs[r].first_pose + j;
      if (pose_inst[p] >= 0) {
        g_last_error = "navgpu_costmap3d_query: two runs share a pose";
        return NAVGPU_ERR_INVALID;
      }
      pose_inst[p] = (int32_t)runs[r].instance;
      const double* q = poses7 + 7 * p;
      const double n2 = q[3] * q[3] + q[4] * q[4] + q[5] * q[5] + q[6] * q[6];
      if (!finite3(q) || !std::isfinite(n2) || !(n2 > 0.0)) {
        g_last_error = "navgpu_costmap3d_query: a pose is not finite or its quaternion is zero";
        return NAVGPU_ERR_INVALID;
      }
      if (regions && regions[p] > NAVGPU_C3D_REGION_RECTANGULAR_PRISM) return NAVGPU_ERR_INVALID;
      if (obstacles && obstacles[p] > NAVGPU_C3D_NONLETHAL) return NAVGPU_ERR_INVALID;
      prism = prism || (regions && regions[p] == NAVGPU_C3D_REGION_RECTANGULAR_PRISM);
    }
  if (prism && (!region_scale || !finite3(region_scale))) return NAVGPU_ERR_INVALID;
  if (!h->have_mesh) {
    g_last_error = "navgpu_costmap3d_query: no mesh (navgpu_costmap3d_set_mesh)";
    return NAVGPU_ERR_STATE;
  }
  if (!n_runs) return NAVGPU_OK;
  int rc = openDevice(h);
  if (rc) return rc;

  const size_t np = (size_t)n_poses;
  const size_t o_inst = 7 * sizeof(double) * np, o_runs = o_inst + sizeof(int32_t) * np, o_reg = o_runs + sizeof(navgpu_c3d_run) * n_runs,
               o_obs = o_reg + np, in_bytes = o_obs + np;
  const size_t o_res = sizeof(double) * np, out_bytes = o_res + sizeof(navgpu_c3d_run_result) * n_runs;
  HIP_TRY(waitStream(h->stream));  // (the staging blocks are free)
  memcpy(h->h_in, poses7, o_inst);
  for (size_t p = 0; p < np; ++p)
    if (pose_inst[p] < 0) std::fill_n(reinterpret_cast<double*>(h->h_in) + 7 * p, 7, 0.0);  // (never read; keep what is uploaded defined)
  memcpy(h->h_in + o_inst, pose_inst.data(), sizeof(int32_t) * np);
  memcpy(h->h_in + o_runs, runs, sizeof(navgpu_c3d_run) * n_runs);
  if (regions) memcpy(h->h_in + o_reg, regions, np); else memset(h->h_in + o_reg, 0, np);
  if (obstacles) memcpy(h->h_in + o_obs, obstacles, np); else memset(h->h_in + o_obs, 0, np);
  HIP_TRY(hipMemcpyAsync(h->d_in, h->h_in, in_bytes, hipMemcpyHostToDevice, h->stream));
  C3dQuery q{};
  q.poses = reinterpret_cast<const double*>(h->d_in);
  q.pose_inst = reinterpret_cast<const int32_t*>(h->d_in + o_inst);
  q.runs = reinterpret_cast<const navgpu_c3d_run*>(h->d_in + o_runs);
  q.regions = h->d_in + o_reg;
  q.obstacles = h->d_in + o_obs;
  q.pose_costs = reinterpret_cast<double*>(h->d_out);
  q.results = reinterpret_cast<navgpu_c3d_run_result*>(h->d_out + o_res);
  q.n_poses = (uint32_t)np;
  q.n_runs = n_runs;
  q.mode = mode;
  q.lazy = lazy ? 1 : 0;
  q.scale_y = region_scale ? region_scale[1] : 0.0;
  q.scale_z = region_scale ? region_scale[2] : 0.0;
  q.limit = distance_limit;
  launch_c3d_query(h->dv, q, h->stream);
  if ((rc = checkLaunch())) return rc;
  HIP_TRY(hipMemcpyAsync(h->h_out, h->d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  const double* costs = reinterpret_cast<const double*>(h->h_out);
  const navgpu_c3d_run_result* res = reinterpret_cast<const navgpu_c3d_run_result*>(h->h_out + o_res);
  if (pose_costs_out)
    for (uint32_t r = 0; r < n_runs; ++r)  // a lazy run's tail stays as the caller left it
      std::copy_n(costs + runs[r].first_pose, (size_t)std::max(res[r].n_done, 0), pose_costs_out + runs[r].first_pose);
  if (results_out) memcpy(results_out, res, sizeof(navgpu_c3d_run_result) * n_runs);
  return NAVGPU_OK;
}

void freeLayers(navgpu_costmap3d* h) {
  if (!h->layered) return;
  for (void* p : h->layered->allocs) hipFree(p);
  if (h->layered->d_grid) hipFree(h->layered->d_grid);
  if (h->layered->h_stage) hipHostFree(h->layered->h_stage);
  delete h->layered;
  h->layered = nullptr;
}

}  // namespace

extern "C" {

int navgpu_costmap3d_create(const navgpu_costmap3d_desc* desc, navgpu_costmap3d** out) {
  if (!desc || !out) return NAVGPU_ERR_INVALID;
  const navgpu_costmap3d_desc& ds = *desc;
  if (!ds.n_instances || !ds.size_x || !ds.size_y || !ds.size_z || ds.size_z > 64 || (uint64_t)ds.size_x * ds.size_y > kC3dMaxColumns ||
      !(ds.resolution > 0.0) || !std::isfinite(ds.resolution) || !ds.max_triangles || ds.max_triangles > NAVGPU_C3D_MAX_TRIANGLES || !ds.max_boxes ||
      !ds.max_poses || ds.device < 0)
    return NAVGPU_ERR_INVALID;
  navgpu_costmap3d* h = new navgpu_costmap3d();
  h->desc = ds;
  h->dv.n = ds.n_instances;
  h->dv.sx = ds.size_x;
  h->dv.sy = ds.size_y;
  h->dv.sz = ds.size_z;
  h->dv.cols = ds.size_x * ds.size_y;
  h->dv.res = ds.resolution;
  h->origins.assign((size_t)ds.n_instances * 3, 0.0);
  *out = h;
  return NAVGPU_OK;
}

int navgpu_costmap3d_destroy(navgpu_costmap3d* h) {
  if (!h) return NAVGPU_ERR_INVALID;
  if (h->opened) {
    (void)hipSetDevice(h->desc.device);
    waitStream(h->stream);
    for (void* p : h->allocs) hipFree(p);
    hipHostFree(h->h_boxes);
    hipHostFree(h->h_in);
    hipHostFree(h->h_out);
    if (h->h_roll) hipHostFree(h->h_roll);
    if (h->pub) {
      for (void* p : {(void*)h->pub->d_shadow, (void*)h->pub->d_stage, (void*)h->pub->d_counts, (void*)h->pub->d_values, (void*)h->pub->d_bounds,
                      (void*)h->pub->d_scratch, (void*)h->pub->d_touched})
        if (p) hipFree(p);
      if (h->pub->h_stage) hipHostFree(h->pub->h_stage);
    }
    freeLayers(h);
    hipStreamDestroy(h->stream);
  }
  delete h->layered;
  delete h->pub;
  delete h;
  return NAVGPU_OK;
}

int navgpu_costmap3d_set_origin(navgpu_costmap3d* h, uint32_t instance, const double origin_xyz[3]) {
  if (!h || !origin_xyz || instance >= h->desc.n_instances || !finite3(origin_xyz)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  if (h->opened) {  // (a handle not opened yet uploads every origin when it is)
    HIP_TRY(hipSetDevice(h->desc.device));
    HIP_TRY(hipMemcpyAsync(h->dv.origins + 3 * (size_t)instance, origin_xyz, sizeof(double) * 3, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(waitStream(h->stream));
  }
  std::copy_n(origin_xyz, 3, h->origins.begin() + 3 * (size_t)instance);
  return NAVGPU_OK;
}

int navgpu_costmap3d_get_origin(navgpu_costmap3d* h, uint32_t instance, double origin_xyz[3]) {
  if (!h || !origin_xyz || instance >= h->desc.n_instances) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  std::copy_n(h->origins.begin() + 3 * (size_t)instance, 3, origin_xyz);
  return NAVGPU_OK;
}

int navgpu_costmap3d_set_boxes(navgpu_costmap3d* h, uint32_t instance, int32_t mode, const navgpu_c3d_box* boxes, uint32_t n, uint32_t* clipped_out) {
  if (!h || instance >= h->desc.n_instances || (n && !boxes) || mode < NAVGPU_C3D_REPLACE || mode > NAVGPU_C3D_CLEAR) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  const navgpu_costmap3d_desc& ds = h->desc;
  if (n > ds.max_boxes) return NAVGPU_ERR_CAPACITY;
  const double* org = h->origins.data() + 3 * (size_t)instance;
  const int64_t size[3] = {ds.size_x, ds.size_y, ds.size_z};
  std::vector<C3dBoxCells> cells;
  cells.reserve(n);
  uint64_t clipped = 0;
  uint32_t max_columns = 0;
  for (uint32_t b = 0; b < n; ++b) {
    const navgpu_c3d_box& bx = boxes[b];
    const double ratio = bx.size / ds.resolution;
    const int k = std::isfinite(ratio) && ratio > 0.5 ? (int)std::nearbyint(std::log2(ratio)) : -1;
    int64_t first[3];
    if (k < 0 || k > 26 || std::fabs(ratio - std::ldexp(1.0, k)) > 1e-6 || (bx.cls != NAVGPU_C3D_LETHAL && bx.cls != NAVGPU_C3D_NONLETHAL) ||
        !alignedCell(bx.cx, bx.size, org[0], ds.resolution, &first[0]) || !alignedCell(bx.cy, bx.size, org[1], ds.resolution, &first[1]) ||
        !alignedCell(bx.cz, bx.size, org[2], ds.resolution, &first[2])) {
      g_last_error = "navgpu_costmap3d_set_boxes: box " + std::to_string(b) + " is not an aligned leaf of the grid (size = resolution * 2^k), or its class is unknown";
      return NAVGPU_ERR_INVALID;
    }
    const int64_t edge = (int64_t)1 << k;
    int64_t lo[3], cnt[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::max<int64_t>(first[a], 0);
      cnt[a] = std::max<int64_t>(std::min<int64_t>(first[a] + edge, size[a]) - lo[a], 0);
    }
    const uint64_t inside = (uint64_t)cnt[0] * (uint64_t)cnt[1] * (uint64_t)cnt[2];
    clipped += (uint64_t)edge * edge * edge - inside;
    if (!inside) continue;
    C3dBoxCells c{};
    c.zmask = (cnt[2] >= 64 ? ~0ull : (((uint64_t)1 << cnt[2]) - 1)) << lo[2];
    c.x0 = (uint32_t)lo[0];
    c.y0 = (uint32_t)lo[1];
    c.nx = (uint32_t)cnt[0];
    c.ny = (uint32_t)cnt[1];
    c.cls = bx.cls;
    max_columns = std::max(max_columns, c.nx * c.ny);
    cells.push_back(c);
  }
  int rc = openDevice(h);
  if (rc) return rc;
  HIP_TRY(waitStream(h->stream));  // (the pinned records of the previous call have been copied)
  if (mode == NAVGPU_C3D_REPLACE)
    HIP_TRY(hipMemsetAsync(h->dv.planes + (size_t)instance * 2 * h->dv.cols, 0, sizeof(uint64_t) * 2 * h->dv.cols, h->stream));
  if (!cells.empty()) {
    std::copy(cells.begin(), cells.end(), h->h_boxes);
    HIP_TRY(hipMemcpyAsync(h->d_boxes, h->h_boxes, sizeof(C3dBoxCells) * cells.size(), hipMemcpyHostToDevice, h->stream));
    launch_c3d_rasterize(h->dv, instance, mode == NAVGPU_C3D_CLEAR ? NAVGPU_C3D_CLEAR : NAVGPU_C3D_MARK, h->d_boxes, (uint32_t)cells.size(), max_columns,
                         h->stream);
    if ((rc = checkLaunch())) return rc;
  }
  if (clipped_out) *clipped_out = (uint32_t)std::min<uint64_t>(clipped, 0xFFFFFFFFull);
  return NAVGPU_OK;  // queued: whatever this handle is asked next runs behind it
}

int navgpu_costmap3d_columns_upload(navgpu_costmap3d* h, uint32_t instance, const uint64_t* lethal, const uint64_t* nonlethal) {
  if (!h || instance >= h->desc.n_instances) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  const size_t cols = h->dv.cols;
  const uint64_t beyond = h->desc.size_z >= 64 ? 0ull : ~0ull << h->desc.size_z;
  for (const uint64_t* plane : {lethal, nonlethal})
    for (size_t c = 0; plane && c < cols; ++c)
      if (plane[c] & beyond) return NAVGPU_ERR_INVALID;
  int rc = openDevice(h);
  if (rc) return rc;
  uint64_t* base = h->dv.planes + (size_t)instance * 2 * cols;
  if (lethal) HIP_TRY(hipMemcpyAsync(base, lethal, sizeof(uint64_t) * cols, hipMemcpyHostToDevice, h->stream));
  if (nonlethal) HIP_TRY(hipMemcpyAsync(base + cols, nonlethal, sizeof(uint64_t) * cols, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));  // the caller's buffers are free again
  return NAVGPU_OK;
}

int navgpu_costmap3d_columns_download(navgpu_costmap3d* h, uint32_t instance, uint64_t* lethal, uint64_t* nonlethal) {
  if (!h || instance >= h->desc.n_instances) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = openDevice(h);
  if (rc) return rc;
  const size_t cols = h->dv.cols;
  const uint64_t* base = h->dv.planes + (size_t)instance * 2 * cols;
  if (lethal) HIP_TRY(hipMemcpyAsync(lethal, base, sizeof(uint64_t) * cols, hipMemcpyDeviceToHost, h->stream));
  if (nonlethal) HIP_TRY(hipMemcpyAsync(nonlethal, base + cols, sizeof(uint64_t) * cols, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_costmap3d_set_mesh(navgpu_costmap3d* h, const double* vertices, uint32_t nv, const uint32_t* triangles, uint32_t nt, double padding,
                              int32_t* closed_out) {
  if (!h || !vertices || !triangles || !nv || !nt || !std::isfinite(padding)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  if (nt > h->desc.max_triangles) return NAVGPU_ERR_CAPACITY;
  std::vector<double> v(vertices, vertices + 3 * (size_t)nv);
  for (double c : v)
    if (!std::isfinite(c)) return NAVGPU_ERR_INVALID;
  if (padding != 0.0)  // padPoints, in float as written there (costmap_3d_query.h:332-350)
    for (uint32_t i = 0; i < nv; ++i) {
      const float x = (float)v[3 * i], y = (float)v[3 * i + 1], pad = (float)padding;
      const float dist = std::sqrt(x * x + y * y);
      if (dist == 0.0f) continue;  // do not pad the origin
      const float nx = x / dist, ny = y / dist;
      v[3 * i] = nx * (dist + pad);
      v[3 * i + 1] = ny * (dist + pad);
    }
  std::vector<double> tri(9 * (size_t)nt);
  std::map<std::pair<uint32_t, uint32_t>, int> directed;  // every directed edge has its opposite exactly once: closed and oriented
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t* ix = triangles + 3 * (size_t)t;
    if (ix[0] >= nv || ix[1] >= nv || ix[2] >= nv) return NAVGPU_ERR_INVALID;
    for (int k = 0; k < 3; ++k) {
      std::copy_n(v.begin() + 3 * (size_t)ix[k], 3, tri.begin() + 9 * (size_t)t + 3 * k);
      ++directed[{ix[k], ix[(k + 1) % 3]}];
    }
    // the edge vectors and the normal: a triangle without area has no place in the separating-axis or the segment tests
    const double* p = tri.data() + 9 * (size_t)t;
    const double e0[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e1[3] = {p[6] - p[3], p[7] - p[4], p[8] - p[5]};
    const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    if (!(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 0.0)) {
      g_last_error = "navgpu_costmap3d_set_mesh: triangle " + std::to_string(t) + " has no area";
      return NAVGPU_ERR_INVALID;
    }
  }
  bool closed = true;
  for (const auto& e : directed) {
    const auto opposite = directed.find({e.first.second, e.first.first});
    closed = closed && e.second == 1 && opposite != directed.end() && opposite->second == 1;
  }
  int rc = openDevice(h);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h->dv.verts, tri.data(), sizeof(double) * tri.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));
  h->dv.nt = nt;
  h->dv.closed = closed ? 1 : 0;
  h->have_mesh = true;
  if (closed_out) *closed_out = closed ? 1 : 0;
  return NAVGPU_OK;
}

int navgpu_costmap3d_query(navgpu_costmap3d* h, uint32_t n_runs, const navgpu_c3d_run* runs, const double* poses, int32_t mode, const uint8_t* regions,
                           const uint8_t* obstacles, const double region_scale[3], double distance_limit, int32_t lazy, double* pose_costs_out,
                           navgpu_c3d_run_result* results_out) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  return runQuery(h, n_runs, runs, poses, mode, regions, obstacles, region_scale, distance_limit, lazy, pose_costs_out, results_out);
}

int navgpu_costmap3d_footprint_costs(navgpu_costmap3d* h, uint32_t n_runs, const navgpu_c3d_run* runs, const double* poses_xyth, double* costs_out,
                                     int32_t* first_illegal_out) {
  if (!h || (n_runs && (!runs || !poses_xyth))) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  uint64_t n_poses = 0;
  for (uint32_t r = 0; r < n_runs; ++r) n_poses = std::max<uint64_t>(n_poses, (uint64_t)runs[r].first_pose + runs[r].n_poses);
  if (n_poses > h->desc.max_poses) return NAVGPU_ERR_CAPACITY;
  std::vector<double> poses7(7 * (size_t)n_poses, 0.0);
  for (uint32_t r = 0; r < n_runs; ++r)
    for (uint32_t j = 0; j < runs[r].n_poses; ++j) {  // tf::createQuaternionMsgFromYaw (costmap_3d_model.cpp:69-72)
      const size_t p = (size_t)runs[r].first_pose + j;
      const double th = poses_xyth[3 * p + 2];
      poses7[7 * p] = poses_xyth[3 * p];
      poses7[7 * p + 1] = poses_xyth[3 * p + 1];
      poses7[7 * p + 5] = std::sin(th * 0.5);
      poses7[7 * p + 6] = std::cos(th * 0.5);
    }
  std::vector<navgpu_c3d_run_result> res(n_runs);
  const int rc = runQuery(h, n_runs, runs, poses7.data(), NAVGPU_C3D_COST, nullptr, nullptr, nullptr, DBL_MAX, 0, costs_out, res.data());
  if (rc) return rc;
  if (first_illegal_out)
    for (uint32_t r = 0; r < n_runs; ++r) first_illegal_out[r] = res[r].first_lethal;
  return NAVGPU_OK;
}

}  // extern "C"

// ---- the layered map update (include/navgpu_costmap3d_layers.h, costmap3d_layer_kernels.hip) ----
namespace {

bool costmapLayer(const navgpu_c3d_layer& l) { return l.kind == NAVGPU_C3D_LAYER_POINT_CLOUD || l.kind == NAVGPU_C3D_LAYER_STATIC_2D; }
bool knownMethod(int32_t m) {
  return m == NAVGPU_C3D_COMBINE_OVERWRITE || m == NAVGPU_C3D_COMBINE_MAXIMUM || m == NAVGPU_C3D_COMBINE_IF_UNKNOWN || m == NAVGPU_C3D_COMBINE_NOTHING;
}

// ok = llround(origin / resolution) per axis; false unless the origin is a multiple of the resolution to 1e-6 of a cell
bool originKeys(const navgpu_costmap3d* h, uint32_t instance, int64_t ok[3]) {
  for (int a = 0; a < 3; ++a) {
    const double f = h->origins[3 * (size_t)instance + a] / h->desc.resolution;
    if (!std::isfinite(f) || std::fabs(f) > 1073741824.0 || std::fabs(f - std::nearbyint(f)) > 1e-6) {
      g_last_error = "costmap3d layers: the origin of instance " + std::to_string(instance) + " is not a multiple of the resolution";
      return false;
    }
    ok[a] = std::llround(f);
  }
  return true;
}

// octomap's coordToKeyClamped less the origin's key
int32_t clampedKey(double c, double inv_res, int64_t ok, uint32_t size) {
  const double k = std::floor(c * inv_res) - (double)ok;
  return k <= 0.0 ? 0 : k >= (double)(size - 1) ? (int32_t)(size - 1) : (int32_t)k;
}

// a call's records, packed into the pinned block behind one another (16-byte aligned) for one upload
struct Stage {
  C3dLayers* L;
  size_t at = 0;
  template <class T>
  size_t put(const T* src, size_t count) {
    const size_t o = at;
    if (count) memcpy(L->h_stage + o, src, sizeof(T) * count);
    at = (o + sizeof(T) * count + 15) & ~(size_t)15;
    return o;
  }
  template <class T>
  T* dev(size_t o) const { return reinterpret_cast<T*>(L->d_stage + o); }
  template <class T>
  T* host(size_t o) const { return reinterpret_cast<T*>(L->h_stage + o); }
};

int layeredHandle(navgpu_costmap3d* h, const char* what) {
  if (h->layered) return NAVGPU_OK;
  g_last_error = std::string(what) + ": navgpu_costmap3d_configure_layers has not been called";
  return NAVGPU_ERR_STATE;
}

// distinct instances below n_instances
int checkInstanceList(const navgpu_costmap3d* h, uint32_t n, const uint32_t* instances) {
  if (n && !instances) return NAVGPU_ERR_INVALID;
  if (n > h->desc.n_instances) return NAVGPU_ERR_INVALID;  // (some instance twice)
  std::vector<uint8_t> seen(h->desc.n_instances, 0);
  for (uint32_t k = 0; k < n; ++k) {
    if (instances[k] >= h->desc.n_instances || seen[instances[k]]) {
      g_last_error = "costmap3d layers: an instance is out of range or listed twice";
      return NAVGPU_ERR_INVALID;
    }
    seen[instances[k]] = 1;
  }
  return NAVGPU_OK;
}

// the first layer call that needs the device: every buffer of the layered update, all or nothing
int openLayers(navgpu_costmap3d* h) {
  int rc = openDevice(h);
  if (rc) return rc;
  C3dLayers* L = h->layered;
  if (L->resident) return NAVGPU_OK;
  C3dLayersDev& ly = L->ly;
  const size_t n = h->desc.n_instances, cols = h->dv.cols, nc = ly.nc;
  // the staging block holds the largest of: a buffer_clouds call's records, an update's, an update_costs call's
  const size_t pairs = n * std::max<size_t>(nc, 1);
  L->stage_bytes = pairs * (sizeof(C3dCloudRec) + 3 * sizeof(uint32_t) + 2 * sizeof(uint32_t)) +
                   n * (sizeof(uint32_t) * (2 + nc) + 3 * sizeof(int64_t) + sizeof(C3dCylRec) * L->n_cyl + 8 * sizeof(int32_t)) + sizeof(C3dGridRec) + 16 * 16;
  auto dalloc = [&](auto** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(**p), 16);
    if (rc) return;
    if (hipMalloc(&q, bytes) != hipSuccess || hipMemsetAsync(q, 0, bytes, h->stream) != hipSuccess) {
      if (q) hipFree(q);
      g_last_error = "hipMalloc failed (costmap3d layers)";
      rc = NAVGPU_ERR_HIP;
      return;
    }
    L->allocs.push_back(q);
    *p = static_cast<std::remove_reference_t<decltype(*p)>>(q);
  };
  dalloc(&ly.sets, n * nc * 2 * 3 * cols);
  dalloc(&ly.changed, n * nc * cols);
  dalloc(&ly.occ, n * nc * 2 * ly.tw);
  dalloc(&ly.dirty, n * ly.tw);
  dalloc(&ly.free_plane, n * cols);
  dalloc(&ly.layer2d, n * cols);
  dalloc(&L->d_stage, L->stage_bytes);
  dalloc(&L->d_points, (size_t)L->max_points * 4);
  if (!rc && hipHostMalloc((void**)&L->h_stage, L->stage_bytes, hipHostMallocDefault) != hipSuccess) {
    L->h_stage = nullptr;
    g_last_error = "hipHostMalloc failed (costmap3d layers)";
    rc = NAVGPU_ERR_HIP;
  }
  if (!rc) {
    launch_c3d_fill_u8(ly.layer2d, 255, n * cols, h->stream);  // NO_INFORMATION
    rc = checkLaunch();
  }
  if (!rc && waitStream(h->stream) != hipSuccess) rc = NAVGPU_ERR_HIP;
  if (rc) {  // the next call starts over
    for (void* q : L->allocs) hipFree(q);
    L->allocs.clear();
    if (L->h_stage) hipHostFree(L->h_stage);
    L->h_stage = nullptr;
    return rc;
  }
  L->resident = true;
  return NAVGPU_OK;
}

// the swap (mode 0) or the touch (mode 1) of the pairs whose records (instance, slot, next) are staged at o_pairs
int queueSwap(navgpu_costmap3d* h, const Stage& st, size_t o_pairs, uint32_t n_pairs, int32_t mode) {
  launch_c3d_layer_swap(h->dv, h->layered->ly, st.dev<uint32_t>(o_pairs), n_pairs, mode, h->stream);
  return checkLaunch();
}

}  // namespace

extern "C" {

int navgpu_costmap3d_configure_layers(navgpu_costmap3d* h, const navgpu_c3d_layer* layers, uint32_t n_layers, int32_t nonlethal_cost_2d) {
  if (!h || !layers || !n_layers || n_layers > NAVGPU_C3D_MAX_LAYERS || nonlethal_cost_2d < 0 || nonlethal_cost_2d > 255) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  std::unique_ptr<C3dLayers> L(new C3dLayers());
  uint32_t nc = 0;
  for (uint32_t l = 0; l < n_layers; ++l) {
    const navgpu_c3d_layer& y = layers[l];
    bool ok = knownMethod(y.combination_method);
    switch (y.kind) {
      case NAVGPU_C3D_LAYER_POINT_CLOUD:
        ok = ok && y.max_cloud_points > 0 &&
             (!y.cloud_has_intensity || (std::isfinite(y.free_intensity) && std::isfinite(y.lethal_intensity) && y.free_intensity != y.lethal_intensity));
        L->max_points = std::max(L->max_points, y.max_cloud_points);
        L->index.push_back(nc++);
        break;
      case NAVGPU_C3D_LAYER_STATIC_2D:
        ok = ok && y.lethal_cost_threshold >= 0 && y.lethal_cost_threshold <= 255 && std::isfinite(y.height);
        L->index.push_back(nc++);
        break;
      case NAVGPU_C3D_LAYER_CYLINDER_CLEARING:
        ok = ok && std::isfinite(y.radius);
        L->index.push_back(L->n_cyl++);
        break;
      default: ok = false;
    }
    if (!ok) {
      g_last_error = "navgpu_costmap3d_configure_layers: layer " + std::to_string(l) + " has an unknown kind or method, or a parameter out of range";
      return NAVGPU_ERR_INVALID;
    }
    L->layers.push_back(y);
    L->layers.back().radius = std::fabs(y.radius);
  }
  const size_t n = h->desc.n_instances;
  if (h->opened) {  // a second call reconfigures from scratch; sizeChange empties the master too (a handle not opened yet has an empty one)
    HIP_TRY(hipSetDevice(h->desc.device));
    HIP_TRY(waitStream(h->stream));
    HIP_TRY(hipMemsetAsync(h->dv.planes, 0, sizeof(uint64_t) * n * 2 * h->dv.cols, h->stream));
  }
  freeLayers(h);
  if (h->pub) h->pub->subs.clear();  // every (instance, layer) subscription starts over (include/navgpu_costmap3d_publish.h)
  C3dLayersDev& ly = L->ly;
  ly.nc = nc;
  ly.tpr = (h->dv.sx + 63) / 64;
  ly.tiles = ly.tpr * h->dv.sy;
  ly.tw = (ly.tiles + 31) / 32;
  ly.nonlethal_cost_2d = nonlethal_cost_2d;
  ly.all_tiles = NAVGPU_DEBUG_ENV("NAVGPU_C3D_ALL_TILES") ? 1 : 0;
  ly.inv_res = 1.0 / h->desc.resolution;
  L->cur.assign(n * nc, 0);
  L->full.assign(n, 1);
  L->moved.assign(n, 0);
  L->prev.assign(n * L->n_cyl, C3dLayers::Cyl());
  h->layered = L.release();
  return NAVGPU_OK;  // the buffers come with the first call that needs the device (openLayers)
}

int navgpu_costmap3d_layer_set(navgpu_costmap3d* h, uint32_t layer, int32_t enabled, int32_t combination_method) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_layer_set");
  if (rc) return rc;
  C3dLayers* L = h->layered;
  if (layer >= L->layers.size() || !knownMethod(combination_method)) return NAVGPU_ERR_INVALID;
  navgpu_c3d_layer& y = L->layers[layer];
  const bool differs = (y.enabled != 0) != (enabled != 0) || y.combination_method != combination_method;
  if (differs && costmapLayer(y) && L->resident) {  // touch: every present cell of the layer, in every instance (nothing is present before the buffers exist)
    const uint32_t slot = L->index[layer];
    std::vector<uint32_t> pairs;
    for (uint32_t i = 0; i < h->desc.n_instances; ++i) {
      const uint32_t c = L->cur[(size_t)i * L->ly.nc + slot];
      pairs.insert(pairs.end(), {i, slot, c ^ 1u});
    }
    HIP_TRY(hipSetDevice(h->desc.device));
    HIP_TRY(waitStream(h->stream));  // (the staging block is free)
    Stage st{L};
    const size_t o = st.put(pairs.data(), pairs.size());
    HIP_TRY(hipMemcpyAsync(L->d_stage, L->h_stage, st.at, hipMemcpyHostToDevice, h->stream));
    if ((rc = queueSwap(h, st, o, h->desc.n_instances, 1))) return rc;
  }
  y.enabled = enabled;
  y.combination_method = combination_method;
  return NAVGPU_OK;
}

int navgpu_costmap3d_buffer_clouds(navgpu_costmap3d* h, const navgpu_c3d_cloud* clouds, uint32_t n_clouds, const float* points, uint32_t n_points,
                                   uint32_t* clipped_out) {
  if (!h || (n_clouds && !clouds) || (n_points && !points)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_buffer_clouds");
  if (rc) return rc;
  C3dLayers* L = h->layered;
  const uint32_t nc = L->ly.nc;
  if (n_points > L->max_points) return NAVGPU_ERR_CAPACITY;
  std::vector<C3dCloudRec> recs(n_clouds);
  std::vector<uint32_t> pairs(3 * (size_t)n_clouds);
  std::vector<uint8_t> seen((size_t)h->desc.n_instances * std::max<uint32_t>(nc, 1), 0);
  uint32_t max_points = 0;
  int format = -1;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    const navgpu_c3d_cloud& c = clouds[k];
    if (c.instance >= h->desc.n_instances || c.layer >= L->layers.size() || L->layers[c.layer].kind != NAVGPU_C3D_LAYER_POINT_CLOUD) {
      g_last_error = "navgpu_costmap3d_buffer_clouds: cloud " + std::to_string(k) + " names no instance or no POINT_CLOUD layer";
      return NAVGPU_ERR_INVALID;
    }
    const navgpu_c3d_layer& y = L->layers[c.layer];
    const uint32_t slot = L->index[c.layer];
    uint8_t& mark = seen[(size_t)c.instance * nc + slot];
    const int fmt = y.cloud_has_intensity ? 1 : 0;
    if (mark || (format >= 0 && fmt != format) || (uint64_t)c.first_point + c.n_points > n_points) {
      g_last_error = "navgpu_costmap3d_buffer_clouds: cloud " + std::to_string(k) +
                     " shares its (instance, layer) with another, mixes point formats, or ends beyond n_points";
      return NAVGPU_ERR_INVALID;
    }
    mark = 1;
    format = fmt;
    for (double v : c.transform)
      if (!std::isfinite(v)) return NAVGPU_ERR_INVALID;
    C3dCloudRec& r = recs[k];
    if (!originKeys(h, c.instance, r.ok)) return NAVGPU_ERR_INVALID;
    std::copy_n(c.transform, 12, r.tf);
    r.instance = c.instance;
    r.slot = slot;
    r.next = L->cur[(size_t)c.instance * nc + slot] ^ 1u;
    r.first_point = c.first_point;
    r.n_points = c.n_points;
    r.has_intensity = (uint32_t)fmt;
    r.free_intensity = y.free_intensity;
    r.lethal_intensity = y.lethal_intensity;
    pairs[3 * (size_t)k] = r.instance;
    pairs[3 * (size_t)k + 1] = r.slot;
    pairs[3 * (size_t)k + 2] = r.next;
    max_points = std::max(max_points, c.n_points);
  }
  if (!n_clouds) return NAVGPU_OK;
  if ((rc = openLayers(h))) return rc;
  HIP_TRY(waitStream(h->stream));  // (the staging block is free)
  Stage st{L};
  const size_t o_recs = st.put(recs.data(), recs.size()), o_pairs = st.put(pairs.data(), pairs.size());
  const std::vector<uint32_t> zeros(n_clouds, 0);
  const size_t o_clip = st.put(zeros.data(), zeros.size());
  HIP_TRY(hipMemcpyAsync(L->d_stage, L->h_stage, st.at, hipMemcpyHostToDevice, h->stream));
  if (n_points) HIP_TRY(hipMemcpyAsync(L->d_points, points, sizeof(float) * (format ? 4 : 3) * (size_t)n_points, hipMemcpyHostToDevice, h->stream));
  launch_c3d_cloud(h->dv, L->ly, st.dev<C3dCloudRec>(o_recs), n_clouds, max_points, L->d_points, st.dev<uint32_t>(o_clip), h->stream);
  if ((rc = checkLaunch())) return rc;
  if ((rc = queueSwap(h, st, o_pairs, n_clouds, 0))) return rc;
  for (uint32_t k = 0; k < n_clouds; ++k) L->cur[(size_t)recs[k].instance * nc + recs[k].slot] = recs[k].next;
  HIP_TRY(hipMemcpyAsync(st.host<uint32_t>(o_clip), st.dev<uint32_t>(o_clip), sizeof(uint32_t) * n_clouds, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));  // (the caller's points are free again)
  if (clipped_out) std::copy_n(st.host<uint32_t>(o_clip), n_clouds, clipped_out);
  return NAVGPU_OK;
}

int navgpu_costmap3d_set_static_grid(navgpu_costmap3d* h, uint32_t instance, uint32_t layer, const int8_t* occupancy, uint32_t width, uint32_t height,
                                     double origin_x, double origin_y, uint32_t* clipped_out) {
  if (!h || !occupancy) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_set_static_grid");
  if (rc) return rc;
  C3dLayers* L = h->layered;
  if (instance >= h->desc.n_instances || layer >= L->layers.size() || L->layers[layer].kind != NAVGPU_C3D_LAYER_STATIC_2D || !width || !height ||
      (uint64_t)width * height > kC3dMaxColumns || !std::isfinite(origin_x) || !std::isfinite(origin_y))
    return NAVGPU_ERR_INVALID;
  const navgpu_c3d_layer& y = L->layers[layer];
  C3dGridRec rec{};
  if (!originKeys(h, instance, rec.ok)) return NAVGPU_ERR_INVALID;
  const size_t cells = (size_t)width * height;
  const uint32_t slot = L->index[layer];
  rec.origin_x = origin_x;
  rec.origin_y = origin_y;
  rec.height = y.height;
  rec.instance = instance;
  rec.slot = slot;
  rec.next = L->cur[(size_t)instance * L->ly.nc + slot] ^ 1u;
  rec.width = width;
  rec.rows = height;
  rec.threshold = y.lethal_cost_threshold;
  rec.unknown_to_lethal = y.unknown_to_lethal ? 1 : 0;
  if ((rc = openLayers(h))) return rc;
  HIP_TRY(waitStream(h->stream));
  if (L->grid_bytes < cells) {
    if (L->d_grid) HIP_TRY(hipFree(L->d_grid));
    L->d_grid = nullptr;
    L->grid_bytes = 0;
    HIP_TRY(hipMalloc((void**)&L->d_grid, cells));
    L->grid_bytes = cells;
  }
  Stage st{L};
  const uint32_t pair[3] = {instance, slot, rec.next}, zero = 0;
  const size_t o_rec = st.put(&rec, 1), o_pair = st.put(pair, 3), o_clip = st.put(&zero, 1);
  HIP_TRY(hipMemcpyAsync(L->d_stage, L->h_stage, st.at, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(L->d_grid, occupancy, cells, hipMemcpyHostToDevice, h->stream));
  launch_c3d_static2d(h->dv, L->ly, st.dev<C3dGridRec>(o_rec), cells, L->d_grid, st.dev<uint32_t>(o_clip), h->stream);
  if ((rc = checkLaunch())) return rc;
  if ((rc = queueSwap(h, st, o_pair, 1, 0))) return rc;
  L->cur[(size_t)instance * L->ly.nc + slot] = rec.next;
  HIP_TRY(hipMemcpyAsync(st.host<uint32_t>(o_clip), st.dev<uint32_t>(o_clip), sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  if (clipped_out) *clipped_out = *st.host<uint32_t>(o_clip);
  return NAVGPU_OK;
}

int navgpu_costmap3d_update(navgpu_costmap3d* h, uint32_t n, const uint32_t* instances, const double* robot_poses_xyz, double* bounds2d_out) {
  if (!h || (n && !robot_poses_xyz)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_update");
  if (rc) return rc;
  if ((rc = checkInstanceList(h, n, instances))) return rc;
  C3dLayers* L = h->layered;
  const uint32_t nc = L->ly.nc, n_cyl = L->n_cyl;
  std::vector<int64_t> ok(3 * (size_t)n);
  std::vector<uint32_t> cur((size_t)n * nc), full(n);
  std::vector<C3dCylRec> cyl((size_t)n * n_cyl);
  std::vector<C3dLayers::Cyl> prev_after((size_t)n * n_cyl);
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = instances[k];
    const double* pose = robot_poses_xyz + 3 * (size_t)k;
    if (!finite3(pose)) {
      g_last_error = "navgpu_costmap3d_update: a robot pose is not finite";
      return NAVGPU_ERR_INVALID;
    }
    if (!originKeys(h, i, ok.data() + 3 * (size_t)k)) return NAVGPU_ERR_INVALID;
    std::copy_n(L->cur.begin() + (size_t)i * nc, nc, cur.begin() + (size_t)k * nc);
    full[k] = L->full[i];
    for (uint32_t l = 0; l < L->layers.size(); ++l) {
      const navgpu_c3d_layer& y = L->layers[l];
      if (y.kind != NAVGPU_C3D_LAYER_CYLINDER_CLEARING) continue;
      const uint32_t c = L->index[l];
      const C3dLayers::Cyl& was = L->prev[(size_t)i * n_cyl + c];
      C3dCylRec& r = cyl[(size_t)k * n_cyl + c];
      const int64_t* o = ok.data() + 3 * (size_t)k;
      auto keyBox = [&](double x, double yy, int32_t* box) {  // coordToKeyClamped of the corners (cylinder_clearing_layer_3d.cpp:98-109)
        box[0] = clampedKey(x - y.radius, L->ly.inv_res, o[0], h->dv.sx);
        box[1] = clampedKey(x + y.radius, L->ly.inv_res, o[0], h->dv.sx);
        box[2] = clampedKey(yy - y.radius, L->ly.inv_res, o[1], h->dv.sy);
        box[3] = clampedKey(yy + y.radius, L->ly.inv_res, o[1], h->dv.sy);
      };
      r = C3dCylRec{};
      r.r = y.radius;
      if (was.has) {
        r.has_prev = 1;
        r.px = was.x;
        r.py = was.y;
        keyBox(was.x, was.y, r.pbox);
      }
      C3dLayers::Cyl& then = prev_after[(size_t)k * n_cyl + c];
      if (y.enabled) {
        r.has_cur = 1;
        r.cx = pose[0];
        r.cy = pose[1];
        keyBox(pose[0], pose[1], r.cbox);
        then.has = true;
        then.x = pose[0];
        then.y = pose[1];
      }  // (else: the previous set is forgotten after it has been added)
    }
  }
  if (!n) return NAVGPU_OK;
  if ((rc = openLayers(h))) return rc;
  HIP_TRY(waitStream(h->stream));  // (the staging block is free)
  Stage st{L};
  std::vector<int32_t> box(4 * (size_t)n);
  for (uint32_t k = 0; k < n; ++k) {
    box[4 * (size_t)k] = box[4 * (size_t)k + 1] = INT32_MAX;
    box[4 * (size_t)k + 2] = box[4 * (size_t)k + 3] = INT32_MIN;
  }
  const size_t o_inst = st.put(instances, n), o_cur = st.put(cur.data(), cur.size()), o_full = st.put(full.data(), n), o_ok = st.put(ok.data(), ok.size()),
               o_cyl = st.put(cyl.data(), cyl.size()), o_box = st.put(box.data(), box.size());
  HIP_TRY(hipMemcpyAsync(L->d_stage, L->h_stage, st.at, hipMemcpyHostToDevice, h->stream));
  C3dUpdate u{};
  u.instances = st.dev<uint32_t>(o_inst);
  u.cur = st.dev<uint32_t>(o_cur);
  u.full = st.dev<uint32_t>(o_full);
  u.ok = st.dev<int64_t>(o_ok);
  u.cyl = st.dev<C3dCylRec>(o_cyl);
  u.box = st.dev<int32_t>(o_box);
  u.n = n;
  u.n_cyl = n_cyl;
  u.n_layers = (uint32_t)L->layers.size();
  for (uint32_t l = 0; l < u.n_layers; ++l)
    u.rules[l] = C3dLayerRule{L->layers[l].kind, L->layers[l].enabled ? 1 : 0, L->layers[l].combination_method, (int32_t)L->index[l]};
  launch_c3d_combine(h->dv, L->ly, u, h->stream);
  if ((rc = checkLaunch())) return rc;
  std::vector<uint8_t> moved(n);
  for (uint32_t k = 0; k < n; ++k) {  // queued: the host's view follows
    L->full[instances[k]] = 0;
    moved[k] = L->moved[instances[k]];
    L->moved[instances[k]] = 0;
    std::copy_n(prev_after.begin() + (size_t)k * n_cyl, n_cyl, L->prev.begin() + (size_t)instances[k] * n_cyl);
  }
  HIP_TRY(hipMemcpyAsync(st.host<int32_t>(o_box), st.dev<int32_t>(o_box), sizeof(int32_t) * 4 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  if (bounds2d_out) {
    const int32_t* got = st.host<int32_t>(o_box);
    const double res = h->desc.resolution;
    for (uint32_t k = 0; k < n; ++k) {  // addExtraBounds of the touched columns, then useExtraBounds (costmap_layer.cpp:34-60)
      const int32_t* b = got + 4 * (size_t)k;
      const double* org = h->origins.data() + 3 * (size_t)instances[k];
      double* out = bounds2d_out + 4 * (size_t)k;
      if (moved[k]) {  // the window itself (costmap_3d_to_2d_layer.cpp:120-127, with maxima where it passes sizes)
        out[0] = org[0];
        out[1] = org[1];
        out[2] = org[0] + h->dv.sx * res;
        out[3] = org[1] + h->dv.sy * res;
      } else if (b[0] > b[2]) {
        out[0] = out[1] = 1e6;
        out[2] = out[3] = -1e6;
      } else {
        out[0] = org[0] + b[0] * res;
        out[1] = org[1] + b[1] * res;
        out[2] = org[0] + (b[2] + 1) * res;
        out[3] = org[1] + (b[3] + 1) * res;
      }
    }
  }
  return NAVGPU_OK;
}

int navgpu_costmap3d_reset(navgpu_costmap3d* h, uint32_t n, const uint32_t* instances) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_reset");
  if (rc) return rc;
  if ((rc = checkInstanceList(h, n, instances))) return rc;
  C3dLayers* L = h->layered;
  const C3dLayersDev& ly = L->ly;
  const size_t cols = h->dv.cols;
  if (n && h->opened) HIP_TRY(hipSetDevice(h->desc.device));
  for (uint32_t k = 0; k < n; ++k) {
    const size_t i = instances[k];
    L->full[i] = 1;
    L->moved[i] = 0;  // (the full flag implies it)
    std::fill_n(L->prev.begin() + i * L->n_cyl, L->n_cyl, C3dLayers::Cyl());
    if (h->opened) HIP_TRY(hipMemsetAsync(h->dv.planes + i * 2 * cols, 0, sizeof(uint64_t) * 2 * cols, h->stream));
    if (!L->resident) continue;  // (nothing else exists yet: it is empty when it does)
    HIP_TRY(hipMemsetAsync(ly.free_plane + i * cols, 0, sizeof(uint64_t) * cols, h->stream));
    if (ly.nc) {
      HIP_TRY(hipMemsetAsync(ly.sets + i * ly.nc * 6 * cols, 0, sizeof(uint64_t) * ly.nc * 6 * cols, h->stream));
      HIP_TRY(hipMemsetAsync(ly.changed + i * ly.nc * cols, 0, sizeof(uint64_t) * ly.nc * cols, h->stream));
      HIP_TRY(hipMemsetAsync(ly.occ + i * ly.nc * 2 * ly.tw, 0, sizeof(uint32_t) * ly.nc * 2 * ly.tw, h->stream));
    }
    HIP_TRY(hipMemsetAsync(ly.dirty + i * ly.tw, 0, sizeof(uint32_t) * ly.tw, h->stream));
  }
  return NAVGPU_OK;  // queued
}

int navgpu_costmap3d_layer2d_download(navgpu_costmap3d* h, uint32_t instance, uint32_t x0, uint32_t y0, uint32_t xn, uint32_t yn, uint8_t* out) {
  if (!h || !out) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_layer2d_download");
  if (rc) return rc;
  if (instance >= h->desc.n_instances || x0 >= xn || y0 >= yn || xn > h->dv.sx || yn > h->dv.sy) return NAVGPU_ERR_INVALID;
  if ((rc = openLayers(h))) return rc;
  const uint8_t* src = h->layered->ly.layer2d + (size_t)instance * h->dv.cols + (size_t)y0 * h->dv.sx + x0;
  HIP_TRY(hipMemcpy2DAsync(out, xn - x0, src, h->dv.sx, xn - x0, yn - y0, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_costmap3d_layer2d_update_costs(navgpu_costmap3d* h, uint32_t n, const uint32_t* instances, void* device_grid, size_t instance_stride_bytes,
                                          uint32_t grid_instances, uint32_t size_x, uint32_t size_y, const int32_t* boxes_ij, int32_t use_maximum) {
  if (!h || !device_grid || (n && !boxes_ij)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_layer2d_update_costs");
  if (rc) return rc;
  if (size_x != h->dv.sx || size_y != h->dv.sy || instance_stride_bytes < (size_t)size_x * size_y) {
    g_last_error = "navgpu_costmap3d_layer2d_update_costs: the grid's size differs from the 3-D map's columns";
    return NAVGPU_ERR_INVALID;
  }
  if ((rc = checkInstanceList(h, n, instances))) return rc;
  for (uint32_t k = 0; k < n; ++k) {
    const int32_t* b = boxes_ij + 4 * (size_t)k;
    if (instances[k] >= grid_instances || b[0] < 0 || b[1] < 0 || b[2] < b[0] || b[3] < b[1] || b[2] > (int32_t)size_x || b[3] > (int32_t)size_y)
      return NAVGPU_ERR_INVALID;
  }
  if (!n) return NAVGPU_OK;
  C3dLayers* L = h->layered;
  if ((rc = openLayers(h))) return rc;
  HIP_TRY(waitStream(h->stream));
  Stage st{L};
  const size_t o_inst = st.put(instances, n), o_box = st.put(boxes_ij, 4 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(L->d_stage, L->h_stage, st.at, hipMemcpyHostToDevice, h->stream));
  C3dCosts2d c{st.dev<uint32_t>(o_inst), st.dev<int32_t>(o_box), static_cast<uint8_t*>(device_grid), instance_stride_bytes, n, use_maximum ? 1 : 0};
  launch_c3d_costs2d(h->dv, L->ly, c, h->stream);
  if ((rc = checkLaunch())) return rc;
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_costmap3d_layer_columns_download(navgpu_costmap3d* h, uint32_t instance, uint32_t layer, uint64_t* lethal, uint64_t* nonlethal,
                                            uint64_t* free_cells, uint64_t* changed) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_layer_columns_download");
  if (rc) return rc;
  C3dLayers* L = h->layered;
  if (instance >= h->desc.n_instances || layer >= L->layers.size() || !costmapLayer(L->layers[layer])) return NAVGPU_ERR_INVALID;
  if ((rc = openLayers(h))) return rc;
  const size_t cols = h->dv.cols, bytes = sizeof(uint64_t) * cols;
  const uint32_t slot = L->index[layer];
  const uint64_t* set = L->ly.set(instance, slot, L->cur[(size_t)instance * L->ly.nc + slot], h->dv.cols);
  if (lethal) HIP_TRY(hipMemcpyAsync(lethal, set + kC3dL * cols, bytes, hipMemcpyDeviceToHost, h->stream));
  if (nonlethal) HIP_TRY(hipMemcpyAsync(nonlethal, set + kC3dN * cols, bytes, hipMemcpyDeviceToHost, h->stream));
  if (free_cells) HIP_TRY(hipMemcpyAsync(free_cells, set + kC3dF * cols, bytes, hipMemcpyDeviceToHost, h->stream));
  if (changed) HIP_TRY(hipMemcpyAsync(changed, L->ly.changed + ((size_t)instance * L->ly.nc + slot) * cols, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_costmap3d_free_columns_download(navgpu_costmap3d* h, uint32_t instance, uint64_t* free_cells) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_free_columns_download");
  if (rc) return rc;
  if (instance >= h->desc.n_instances) return NAVGPU_ERR_INVALID;
  if ((rc = openLayers(h))) return rc;
  if (free_cells)
    HIP_TRY(hipMemcpyAsync(free_cells, h->layered->ly.free_plane + (size_t)instance * h->dv.cols, sizeof(uint64_t) * h->dv.cols, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

}  // extern "C"

// ---- rolling maps and resetBoundingBox (include/navgpu_costmap3d_rolling.h, costmap3d_roll_kernels.hip) ----
namespace {

static_assert(sizeof(C3dRollRec) == 32 && sizeof(C3dResetRec) == 32, "one staging block serves both record types");

// the records of a roll or a reset_bounding_box call: a device block and its pinned twin, one record per instance
int openRollStage(navgpu_costmap3d* h) {
  if (h->d_roll) return NAVGPU_OK;
  const size_t bytes = sizeof(C3dRollRec) * h->desc.n_instances;
  if (hipHostMalloc((void**)&h->h_roll, bytes, hipHostMallocDefault) != hipSuccess) {
    h->h_roll = nullptr;
    g_last_error = "hipHostMalloc failed (costmap3d roll)";
    return NAVGPU_ERR_HIP;
  }
  const int rc = h->alloc(&h->d_roll, bytes);
  if (rc) {
    hipHostFree(h->h_roll);
    h->h_roll = nullptr;
  }
  return rc;
}

// bit s: the current plane set of slot s
uint32_t currentSets(const C3dLayers* L, uint32_t instance) {
  uint32_t bits = 0;
  for (uint32_t s = 0; L && s < L->ly.nc; ++s) bits |= (L->cur[(size_t)instance * L->ly.nc + s] & 1u) << s;
  return bits;
}

}  // namespace

extern "C" {

int navgpu_costmap3d_roll(navgpu_costmap3d* h, uint32_t n, const uint32_t* instances, int32_t mode, const double* targets_xy, int32_t* shifts_out) {
  if (!h || (n && !targets_xy) || (mode != NAVGPU_C3D_ROLL_CENTRE && mode != NAVGPU_C3D_ROLL_ORIGIN)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = checkInstanceList(h, n, instances);
  if (rc) return rc;
  C3dLayers* L = h->layered;
  const double res = h->desc.resolution;
  const uint32_t size[2] = {h->dv.sx, h->dv.sy};
  std::vector<C3dRollRec> recs;
  std::vector<int32_t> shifts(2 * (size_t)n);
  bool any_y = false, any_x = false;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = instances[k];
    const double* t = targets_xy + 2 * (size_t)k;
    if (!std::isfinite(t[0]) || !std::isfinite(t[1])) {
      g_last_error = "navgpu_costmap3d_roll: a target is not finite";
      return NAVGPU_ERR_INVALID;
    }
    int64_t ok[3], shift[2];
    if (!originKeys(h, i, ok)) return NAVGPU_ERR_INVALID;
    double key[2];
    for (int a = 0; a < 2; ++a) {
      if (mode == NAVGPU_C3D_ROLL_CENTRE) {  // LayeredCostmap3D::updateMap with octomap::point3d's floats (layered_costmap_3d.cpp:78-92)
        const double w = (double)(float)(size[a] * res);
        const float m = (float)(t[a] - w / 2.0);
        key[a] = std::floor((double)m * (1.0 / res));
      } else {
        const double f = t[a] / res;
        key[a] = std::nearbyint(f);
        if (!std::isfinite(f) || std::fabs(f - key[a]) > 1e-6) {
          g_last_error = "navgpu_costmap3d_roll: the new origin of instance " + std::to_string(i) + " is not a multiple of the resolution";
          return NAVGPU_ERR_INVALID;
        }
      }
      if (!(std::fabs(key[a]) <= 1073741824.0)) {
        g_last_error = "navgpu_costmap3d_roll: the new window of instance " + std::to_string(i) + " lies beyond the keys an origin may have";
        return NAVGPU_ERR_INVALID;
      }
      shift[a] = (int64_t)key[a] - ok[a];
      shifts[2 * (size_t)k + a] = (int32_t)std::max<int64_t>(std::min<int64_t>(shift[a], INT32_MAX), INT32_MIN);
    }
    if (!shift[0] && !shift[1]) continue;  // not touched, no moved mark
    C3dRollRec r{};
    r.ox = key[0] * res;
    r.oy = key[1] * res;
    r.instance = i;
    r.cur_bits = currentSets(L, i);
    if (std::llabs(shift[0]) >= (int64_t)size[0] || std::llabs(shift[1]) >= (int64_t)size[1]) {
      r.cur_bits |= kC3dRollEmpty;
      any_x = true;  // (the fill goes by rows)
    } else {
      r.dx = (int32_t)shift[0];
      r.dy = (int32_t)shift[1];
      any_x = any_x || r.dx;
      any_y = any_y || r.dy;
    }
    recs.push_back(r);
  }
  if (!recs.empty()) {
    if ((rc = L ? openLayers(h) : openDevice(h))) return rc;
    if ((rc = openRollStage(h))) return rc;
    HIP_TRY(waitStream(h->stream));  // (the staging block is free)
    memcpy(h->h_roll, recs.data(), sizeof(C3dRollRec) * recs.size());
    HIP_TRY(hipMemcpyAsync(h->d_roll, h->h_roll, sizeof(C3dRollRec) * recs.size(), hipMemcpyHostToDevice, h->stream));
    launch_c3d_roll(h->dv, L ? L->ly : C3dLayersDev{}, L ? 1 : 0, reinterpret_cast<const C3dRollRec*>(h->d_roll), (uint32_t)recs.size(), any_y, any_x,
                    h->stream);
    if ((rc = checkLaunch())) return rc;
    for (const C3dRollRec& r : recs) {  // queued: the host's view follows
      h->origins[3 * (size_t)r.instance] = r.ox;
      h->origins[3 * (size_t)r.instance + 1] = r.oy;
      if (L) L->moved[r.instance] = 1;
    }
  }
  if (shifts_out) std::copy(shifts.begin(), shifts.end(), shifts_out);
  return NAVGPU_OK;
}

int navgpu_costmap3d_reset_bounding_box(navgpu_costmap3d* h, uint32_t n, const uint32_t* instances, const double* boxes, uint32_t layer_mask) {
  if (!h || (n && !boxes)) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_reset_bounding_box");
  if (rc) return rc;
  if ((rc = checkInstanceList(h, n, instances))) return rc;
  C3dLayers* L = h->layered;
  if (L->layers.size() < 32 && (layer_mask >> L->layers.size())) {
    g_last_error = "navgpu_costmap3d_reset_bounding_box: layer_mask names a layer that is not configured";
    return NAVGPU_ERR_INVALID;
  }
  C3dResetSlots slots{};
  for (uint32_t l = 0; l < L->layers.size(); ++l)  // a STATIC_2D layer ignores the call (static_2d_layer_3d.cpp:153-158); a cylinder layer keeps its set
    if (((layer_mask >> l) & 1u) && L->layers[l].kind == NAVGPU_C3D_LAYER_POINT_CLOUD) slots.slot[slots.n++] = L->index[l];
  const uint32_t size[3] = {h->dv.sx, h->dv.sy, h->dv.sz};
  std::vector<C3dResetRec> recs;
  uint32_t max_tiles = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const double* b = boxes + 6 * (size_t)k;
    if (!finite3(b) || !finite3(b + 3)) {
      g_last_error = "navgpu_costmap3d_reset_bounding_box: a box is not finite";
      return NAVGPU_ERR_INVALID;
    }
    int64_t ok[3];
    if (!originKeys(h, instances[k], ok)) return NAVGPU_ERR_INVALID;
    uint32_t lo[3], hi[3];
    bool empty = false;
    for (int a = 0; a < 3; ++a) {  // the keys of the corners, both ends inclusive (costmap_layer_3d.cpp:149-191), clipped to the window
      const double k0 = std::floor(b[a] * L->ly.inv_res) - (double)ok[a], k1 = std::floor(b[3 + a] * L->ly.inv_res) - (double)ok[a];
      if (b[a] > b[3 + a] || k1 < 0.0 || k0 > (double)(size[a] - 1)) {
        empty = true;
        break;
      }
      lo[a] = k0 <= 0.0 ? 0u : (uint32_t)k0;
      hi[a] = k1 >= (double)(size[a] - 1) ? size[a] - 1 : (uint32_t)k1;
    }
    if (empty) continue;
    C3dResetRec r{};
    const uint32_t levels = hi[2] - lo[2] + 1;
    r.zmask = (levels >= 64 ? ~0ull : ((uint64_t)1 << levels) - 1) << lo[2];
    r.instance = instances[k];
    r.cur_bits = currentSets(L, instances[k]);
    r.x0 = lo[0];
    r.x1 = hi[0];
    r.y0 = lo[1];
    r.y1 = hi[1];
    max_tiles = std::max(max_tiles, ((r.x1 >> 6) - (r.x0 >> 6) + 1) * (r.y1 - r.y0 + 1));
    recs.push_back(r);
  }
  if (recs.empty() || !slots.n) return NAVGPU_OK;
  if ((rc = openLayers(h))) return rc;
  if ((rc = openRollStage(h))) return rc;
  HIP_TRY(waitStream(h->stream));  // (the staging block is free)
  memcpy(h->h_roll, recs.data(), sizeof(C3dResetRec) * recs.size());
  HIP_TRY(hipMemcpyAsync(h->d_roll, h->h_roll, sizeof(C3dResetRec) * recs.size(), hipMemcpyHostToDevice, h->stream));
  launch_c3d_reset_box(h->dv, L->ly, reinterpret_cast<const C3dResetRec*>(h->d_roll), (uint32_t)recs.size(), max_tiles, slots, h->stream);
  return checkLaunch();  // queued
}

}  // extern "C"

// ---- publishing: pruned octree leaves out of a handle and into a layer (include/navgpu_costmap3d_publish.h, costmap3d_publish_kernels.hip) ----
namespace {

static_assert(sizeof(navgpu_c3d_leaf) == 16 && sizeof(navgpu_c3d_update_msg) == 88, "the records of include/navgpu_costmap3d_publish.h");

C3dPublish* publishState(navgpu_costmap3d* h) {
  if (!h->pub) h->pub = new C3dPublish();
  return h->pub;
}

// a device block of at least `want` items; a block that grows is new and, with zero, all zero
template <class T>
int growDevice(navgpu_costmap3d* h, T** p, size_t* have, size_t want, bool zero) {
  if (*have >= want && *p) return NAVGPU_OK;
  if (*p) {
    HIP_TRY(waitStream(h->stream));
    HIP_TRY(hipFree(*p));
  }
  *p = nullptr;
  *have = 0;
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(want * sizeof(T), 16);
  if (hipMalloc(&q, bytes) != hipSuccess) {
    g_last_error = "hipMalloc failed (costmap3d publish)";
    return NAVGPU_ERR_HIP;
  }
  if (zero && hipMemsetAsync(q, 0, bytes, h->stream) != hipSuccess) {
    hipFree(q);
    return NAVGPU_ERR_HIP;
  }
  *p = static_cast<T*>(q);
  *have = want;
  return NAVGPU_OK;
}

int growStage(navgpu_costmap3d* h, size_t bytes) {
  C3dPublish* P = h->pub;
  if (P->stage_bytes >= bytes && P->d_stage) return NAVGPU_OK;
  HIP_TRY(waitStream(h->stream));
  if (P->h_stage) hipHostFree(P->h_stage);
  P->h_stage = nullptr;
  size_t have = P->d_stage ? P->stage_bytes : 0;
  P->stage_bytes = 0;
  int rc = growDevice(h, &P->d_stage, &have, bytes, false);
  if (rc) return rc;
  if (hipHostMalloc((void**)&P->h_stage, std::max<size_t>(bytes, 16), hipHostMallocDefault) != hipSuccess) {
    P->h_stage = nullptr;
    hipFree(P->d_stage);
    P->d_stage = nullptr;
    g_last_error = "hipHostMalloc failed (costmap3d publish)";
    return NAVGPU_ERR_HIP;
  }
  P->stage_bytes = bytes;
  return NAVGPU_OK;
}

int64_t floorDiv64(int64_t v) { return v >= 0 ? v / 64 : -((-v + 63) / 64); }

// shadow window \ current window as at most two lattice boxes: the x strip over the old y range, the y strip over the remaining x range
uint32_t forgottenBoxes(const int64_t* was, const int64_t* now, const int64_t* size, int32_t out[2][6]) {
  uint32_t n = 0;
  const int64_t x_end = was[0] + size[0] - 1, y_end = was[1] + size[1] - 1;
  auto put = [&](int64_t x0, int64_t x1, int64_t y0, int64_t y1) {
    const int64_t box[6] = {x0, y0, was[2], x1, y1, was[2] + size[2] - 1};
    for (int a = 0; a < 6; ++a) out[n][a] = (int32_t)box[a];
    ++n;
  };
  if (now[0] > was[0]) put(was[0], std::min(now[0] - 1, x_end), was[1], y_end);
  else if (now[0] < was[0]) put(std::max(now[0] + size[0], was[0]), x_end, was[1], y_end);
  const int64_t x0 = std::max(was[0], now[0]), x1 = std::min(was[0], now[0]) + size[0] - 1;  // the x range both windows hold
  if (x0 <= x1) {
    if (now[1] > was[1]) put(x0, x1, was[1], std::min(now[1] - 1, y_end));
    else if (now[1] < was[1]) put(x0, x1, std::max(now[1] + size[1], was[1]), y_end);
  }
  return n;
}

}  // namespace

extern "C" {

int navgpu_costmap3d_publisher_configure(navgpu_costmap3d* h, int32_t enabled) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  C3dPublish* P = publishState(h);
  const size_t n = h->desc.n_instances;
  if (P->d_shadow) {  // shadows start empty
    HIP_TRY(hipSetDevice(h->desc.device));
    HIP_TRY(hipMemsetAsync(P->d_shadow, 0, sizeof(uint64_t) * n * P->shadow_planes * h->dv.cols, h->stream));
  }
  P->enabled = enabled != 0;
  P->seq.assign(P->enabled ? n : 0, 0);
  P->window.assign(P->enabled ? 3 * n : 0, 0);
  P->has_window.assign(P->enabled ? n : 0, 0);
  return NAVGPU_OK;
}

int navgpu_costmap3d_export(navgpu_costmap3d* h, uint32_t n, const uint32_t* instances, int32_t mode, uint32_t value_capacity, navgpu_c3d_leaf* values,
                            uint32_t bounds_capacity, navgpu_c3d_leaf* bounds, navgpu_c3d_update_msg* msgs) {
  if (!h || !msgs || (mode != NAVGPU_C3D_EXPORT_FULL && mode != NAVGPU_C3D_EXPORT_DELTA) || (value_capacity && !values) || (bounds_capacity && !bounds))
    return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = checkInstanceList(h, n, instances);
  if (rc) return rc;
  const bool delta = mode == NAVGPU_C3D_EXPORT_DELTA, layered = h->layered != nullptr;
  const int64_t size[3] = {h->dv.sx, h->dv.sy, h->dv.sz};
  std::vector<C3dExportRec> recs(n);
  std::vector<int64_t> ok(3 * (size_t)n);
  uint32_t blocks = 0, max_blocks = 0;
  for (uint32_t k = 0; k < n; ++k) {
    int64_t* o = ok.data() + 3 * (size_t)k;
    if (!originKeys(h, instances[k], o)) return NAVGPU_ERR_INVALID;  // (|key| <= 2^30 and size < 2^26: the window fits int32_t)
    C3dExportRec& r = recs[k];
    r = C3dExportRec{};
    for (int a = 0; a < 3; ++a) r.ok[a] = (int32_t)o[a];
    r.bx0 = (int32_t)floorDiv64(o[0]);
    r.by0 = (int32_t)floorDiv64(o[1]);
    r.nbx = (uint32_t)(floorDiv64(o[0] + size[0] - 1) - r.bx0 + 1);
    r.nby = (uint32_t)(floorDiv64(o[1] + size[1] - 1) - r.by0 + 1);
    r.instance = instances[k];
    r.first_block = blocks;
    blocks += r.nbx * r.nby;
    max_blocks = std::max(max_blocks, r.nbx * r.nby);
  }
  if (delta && !(h->pub && h->pub->enabled)) {
    g_last_error = "navgpu_costmap3d_export: DELTA needs navgpu_costmap3d_publisher_configure";
    return NAVGPU_ERR_STATE;
  }
  if (!n) return NAVGPU_OK;
  C3dPublish* P = publishState(h);
  const bool sequenced = P->enabled;
  for (uint32_t k = 0; k < n && delta; ++k) {  // where the shadow lies; one without a window is empty, wherever it is read
    const uint32_t i = instances[k];
    for (int a = 0; a < 3; ++a) {
      const int64_t d = P->has_window[i] ? ok[3 * (size_t)k + a] - P->window[3 * (size_t)i + a] : 0;
      recs[k].sd[a] = (int32_t)std::max<int64_t>(std::min<int64_t>(d, INT32_MAX / 2), INT32_MIN / 2);  // (beyond the window either way)
    }
  }
  if ((rc = layered ? openLayers(h) : openDevice(h))) return rc;
  const uint32_t np = layered ? 3u : 2u;
  const size_t cols = h->dv.cols, n_all = h->desc.n_instances;
  if (delta && (!P->d_shadow || P->shadow_planes != np)) {  // (configure_layers since: the master was emptied with it)
    size_t have = 0;
    if (P->d_shadow) {
      HIP_TRY(waitStream(h->stream));
      HIP_TRY(hipFree(P->d_shadow));
      P->d_shadow = nullptr;
    }
    if ((rc = growDevice(h, &P->d_shadow, &have, n_all * np * cols, true))) return rc;
    P->shadow_planes = np;
  }
  const size_t o_totals = (sizeof(C3dExportRec) * n + 15) & ~(size_t)15;
  if ((rc = growStage(h, o_totals + sizeof(uint32_t) * 4 * n))) return rc;
  if ((rc = growDevice(h, &P->d_counts, &P->count_words, 4 * (size_t)blocks + 4 * (size_t)n, false))) return rc;
  HIP_TRY(waitStream(h->stream));  // (the staging block is free)
  memcpy(P->h_stage, recs.data(), sizeof(C3dExportRec) * n);
  HIP_TRY(hipMemcpyAsync(P->d_stage, P->h_stage, sizeof(C3dExportRec) * n, hipMemcpyHostToDevice, h->stream));
  C3dExport e{};
  e.recs = reinterpret_cast<const C3dExportRec*>(P->d_stage);
  e.shadow = P->d_shadow;
  e.counts = P->d_counts;
  e.offsets = P->d_counts + 2 * (size_t)blocks;
  e.totals = P->d_counts + 4 * (size_t)blocks;
  e.n = n;
  e.blocks = blocks;
  e.max_blocks = max_blocks;
  e.np = np;
  e.delta = delta ? 1 : 0;
  const C3dLayersDev ly = layered ? h->layered->ly : C3dLayersDev{};
  launch_c3d_export_count(h->dv, ly, e, h->stream);
  if ((rc = checkLaunch())) return rc;
  uint32_t* totals = reinterpret_cast<uint32_t*>(P->h_stage + o_totals);
  HIP_TRY(hipMemcpyAsync(totals, e.totals, sizeof(uint32_t) * 4 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  uint64_t n_values = 0, n_bounds = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = instances[k];
    navgpu_c3d_update_msg& m = msgs[k];
    m = navgpu_c3d_update_msg{};
    m.instance = i;
    m.update_seq = sequenced ? P->seq[i] : 0u;
    m.bounds_seq = delta || !sequenced ? m.update_seq : m.update_seq - 1u;  // (the sentinel of a first map, costmap_3d_publisher.cpp:139-143)
    m.universe = delta ? 0 : 1;
    m.first_value = totals[4 * k];
    m.n_values = totals[4 * k + 1];
    m.first_bound = totals[4 * k + 2];
    m.n_bounds = totals[4 * k + 3];
    if (delta && P->has_window[i]) m.n_forgotten = forgottenBoxes(P->window.data() + 3 * (size_t)i, ok.data() + 3 * (size_t)k, size, m.forgotten);
    n_values += m.n_values;
    n_bounds += m.n_bounds;
  }
  if (!values && !bounds) return NAVGPU_OK;  // counted only: nothing is committed
  if (n_values > value_capacity || n_bounds > bounds_capacity) {
    g_last_error = "navgpu_costmap3d_export: " + std::to_string(n_values) + " value and " + std::to_string(n_bounds) + " bounds leaves exceed the capacities";
    return NAVGPU_ERR_CAPACITY;
  }
  if ((rc = growDevice(h, &P->d_values, &P->value_capacity, (size_t)n_values, false))) return rc;
  if ((rc = growDevice(h, &P->d_bounds, &P->bounds_capacity, (size_t)n_bounds, false))) return rc;
  e.values = P->d_values;
  e.bounds = P->d_bounds;
  e.value_capacity = (uint32_t)n_values;
  e.bounds_capacity = (uint32_t)n_bounds;
  if (n_values || n_bounds) {
    launch_c3d_export_emit(h->dv, ly, e, h->stream);
    if ((rc = checkLaunch())) return rc;
  }
  if (delta) {
    launch_c3d_shadow_copy(h->dv, ly, e, P->d_shadow, h->stream);
    if ((rc = checkLaunch())) return rc;
  }
  if (n_values) HIP_TRY(hipMemcpyAsync(values, P->d_values, sizeof(navgpu_c3d_leaf) * (size_t)n_values, hipMemcpyDeviceToHost, h->stream));
  if (n_bounds) HIP_TRY(hipMemcpyAsync(bounds, P->d_bounds, sizeof(navgpu_c3d_leaf) * (size_t)n_bounds, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  for (uint32_t k = 0; k < n && delta; ++k) {  // published: the host's view follows
    const uint32_t i = instances[k];
    ++P->seq[i];
    P->has_window[i] = 1;
    std::copy_n(ok.begin() + 3 * (size_t)k, 3, P->window.begin() + 3 * (size_t)i);
  }
  return NAVGPU_OK;
}

int navgpu_costmap3d_layer_resubscribe(navgpu_costmap3d* h, uint32_t instance, uint32_t layer) {
  if (!h) return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_layer_resubscribe");
  if (rc) return rc;
  C3dLayers* L = h->layered;
  if (instance >= h->desc.n_instances || layer >= L->layers.size() || !costmapLayer(L->layers[layer])) return NAVGPU_ERR_INVALID;
  C3dPublish* P = publishState(h);
  if (P->subs_of == L && !P->subs.empty()) P->subs[(size_t)instance * L->ly.nc + L->index[layer]] = C3dPublish::Sub();
  return NAVGPU_OK;  // (states that do not exist yet start over by themselves)
}

int navgpu_costmap3d_layer_update_cells(navgpu_costmap3d* h, uint32_t n_msgs, const navgpu_c3d_update_msg* msgs, const uint32_t* layers, int32_t cell_mode,
                                        const navgpu_c3d_leaf* values, uint32_t n_values, const navgpu_c3d_leaf* bounds, uint32_t n_bounds,
                                        int32_t* verdicts_out) {
  if (!h || !msgs || !layers || (cell_mode != NAVGPU_C3D_CELLS_BINARY && cell_mode != NAVGPU_C3D_CELLS_AS_GIVEN) || (n_values && !values) ||
      (n_bounds && !bounds))
    return NAVGPU_ERR_INVALID;
  C3dGuard guard_(h);
  int rc = layeredHandle(h, "navgpu_costmap3d_layer_update_cells");
  if (rc) return rc;
  if ((uint64_t)n_values + n_bounds > h->desc.max_boxes) {
    g_last_error = "navgpu_costmap3d_layer_update_cells: " + std::to_string((uint64_t)n_values + n_bounds) + " leaves exceed max_boxes";
    return NAVGPU_ERR_CAPACITY;
  }
  C3dLayers* L = h->layered;
  C3dPublish* P = publishState(h);
  const uint32_t nc = L->ly.nc;
  std::vector<C3dPublish::Sub> subs = P->subs_of == L && P->subs.size() == (size_t)h->desc.n_instances * nc
                                          ? P->subs
                                          : std::vector<C3dPublish::Sub>((size_t)h->desc.n_instances * nc);  // (a configure_layers resets them all)
  std::vector<uint8_t> seen(subs.size(), 0);
  std::vector<int32_t> verdicts(n_msgs);
  std::vector<C3dCellsMsg> applied;
  std::vector<C3dBoxCells> leaves;
  const int64_t size[3] = {h->dv.sx, h->dv.sy, h->dv.sz};
  uint32_t max_columns = 0;
  auto bad = [&](uint32_t k, const char* why) {
    g_last_error = "navgpu_costmap3d_layer_update_cells: message " + std::to_string(k) + ": " + why;
    return NAVGPU_ERR_INVALID;
  };
  // the clipped cells of a lattice box [lo, lo + cnt) per axis; false: none inside the window
  auto clip = [&](const int64_t* ok, const int64_t* lo, const int64_t* cnt, C3dBoxCells* c) {
    int64_t first[3], count[3];
    for (int a = 0; a < 3; ++a) {
      first[a] = std::max<int64_t>(lo[a] - ok[a], 0);
      count[a] = std::min<int64_t>(lo[a] - ok[a] + cnt[a], size[a]) - first[a];
      if (count[a] <= 0) return false;
    }
    c->zmask = (count[2] >= 64 ? ~0ull : (((uint64_t)1 << count[2]) - 1)) << first[2];
    c->x0 = (uint32_t)first[0];
    c->y0 = (uint32_t)first[1];
    c->nx = (uint32_t)count[0];
    c->ny = (uint32_t)count[1];
    return true;
  };
  for (uint32_t k = 0; k < n_msgs; ++k) {
    const navgpu_c3d_update_msg& m = msgs[k];
    if (m.instance >= h->desc.n_instances || layers[k] >= L->layers.size() || !costmapLayer(L->layers[layers[k]])) return bad(k, "names no instance or no costmap layer");
    const uint32_t slot = L->index[layers[k]];
    const size_t pair = (size_t)m.instance * nc + slot;
    if (seen[pair]) return bad(k, "shares its (instance, layer) with another");
    seen[pair] = 1;
    if ((uint64_t)m.first_value + m.n_values > n_values || (uint64_t)m.first_bound + m.n_bounds > n_bounds) return bad(k, "a range ends beyond its array");
    if (m.n_forgotten > 2) return bad(k, "n_forgotten > 2");
    for (uint32_t f = 0; f < m.n_forgotten; ++f)
      for (int a = 0; a < 3; ++a)
        if (m.forgotten[f][3 + a] < m.forgotten[f][a]) return bad(k, "a forgotten box is inverted");
    auto leafOk = [](const navgpu_c3d_leaf& l) {
      if (l.level > 6 || l.cls > NAVGPU_C3D_FREE) return false;
      const int32_t mask = (1 << l.level) - 1;
      return !((l.key[0] | l.key[1] | l.key[2]) & mask);  // (two's complement: a multiple of 2^level, floor-mod)
    };
    for (uint32_t j = 0; j < m.n_values; ++j)
      if (!leafOk(values[m.first_value + j])) return bad(k, "a value leaf has a key not aligned to its level, a level > 6 or an unknown class");
    for (uint32_t j = 0; j < m.n_bounds; ++j)
      if (!leafOk(bounds[m.first_bound + j])) return bad(k, "a bounds leaf has a key not aligned to its level, a level > 6 or an unknown class");
    int64_t ok[3];
    if (!originKeys(h, m.instance, ok)) return NAVGPU_ERR_INVALID;
    // mapCallback / mapUpdateCallback (octomap_server_layer_3d.cpp:281-350)
    C3dPublish::Sub& s = subs[pair];
    if (m.plain_map) {
      if (s.using_updates) {
        verdicts[k] = NAVGPU_C3D_IGNORED;
        continue;
      }
    } else {
      ++s.n_updates;
      if (!s.first_full) {
        if (s.n_updates == 1 && m.bounds_seq == m.update_seq) {
          verdicts[k] = NAVGPU_C3D_IGNORED;
          continue;
        }
        if (s.n_updates > 1) {  // the first full map was lost: subscribeUpdatesUnlocked (:179-186)
          s.first_full = false;
          s.n_updates = 0;
          verdicts[k] = NAVGPU_C3D_RESYNC;
          continue;
        }
        s.first_full = true;
      } else if ((uint32_t)(s.last_seq + 1u) < m.bounds_seq) {
        s.first_full = false;
        s.n_updates = 0;
        verdicts[k] = NAVGPU_C3D_RESYNC;
        continue;
      }
      s.last_seq = m.bounds_seq;
      s.using_updates = true;
    }
    verdicts[k] = NAVGPU_C3D_APPLIED;
    C3dCellsMsg rec{};
    rec.instance = m.instance;
    rec.slot = slot;
    rec.cur = L->cur[pair];
    const bool universe = m.universe || m.plain_map;
    uint32_t n_forgotten = 0;
    for (uint32_t f = 0; f < m.n_forgotten && !universe; ++f) {
      int64_t lo[3], cnt[3];
      for (int a = 0; a < 3; ++a) {
        lo[a] = m.forgotten[f][a];
        cnt[a] = (int64_t)m.forgotten[f][3 + a] - m.forgotten[f][a] + 1;
      }
      C3dBoxCells c{};
      if (!clip(ok, lo, cnt, &c)) continue;
      rec.fz[n_forgotten] = c.zmask;
      const int32_t box[4] = {(int32_t)c.x0, (int32_t)(c.x0 + c.nx - 1), (int32_t)c.y0, (int32_t)(c.y0 + c.ny - 1)};
      std::copy_n(box, 4, rec.fbox[n_forgotten]);
      ++n_forgotten;
    }
    rec.flags = (universe ? 1u : 0u) | (n_forgotten << 1);
    const size_t leaves_before = leaves.size();
    auto put = [&](const navgpu_c3d_leaf& l, int32_t plane) {
      const int64_t lo[3] = {l.key[0], l.key[1], l.key[2]}, edge = (int64_t)1 << l.level, cnt[3] = {edge, edge, edge};
      C3dBoxCells c{};
      if (!clip(ok, lo, cnt, &c)) return;
      c.cls = plane;
      c.reserved = (int32_t)applied.size();
      max_columns = std::max(max_columns, c.nx * c.ny);
      leaves.push_back(c);
    };
    for (uint32_t j = 0; j < m.n_bounds && !universe; ++j) put(bounds[m.first_bound + j], 0);
    for (uint32_t j = 0; j < m.n_values; ++j) {
      const navgpu_c3d_leaf& l = values[m.first_value + j];
      put(l, 1 + (cell_mode == NAVGPU_C3D_CELLS_BINARY && l.cls == NAVGPU_C3D_NONLETHAL ? (int32_t)NAVGPU_C3D_LETHAL : (int32_t)l.cls));
    }
    if (rec.flags || leaves.size() != leaves_before) applied.push_back(rec);  // (an empty delta, or one wholly off the window, queues nothing)
  }
  if (!applied.empty()) {
    if ((rc = openLayers(h))) return rc;
    const size_t o_leaves = sizeof(C3dCellsMsg) * applied.size(), bytes = o_leaves + sizeof(C3dBoxCells) * leaves.size();
    if ((rc = growStage(h, bytes))) return rc;
    if (P->scratch_msgs < applied.size() || !P->d_scratch || !P->d_touched) {
      size_t a = P->d_scratch ? P->scratch_msgs : 0, b = P->d_touched ? P->scratch_msgs : 0;
      P->scratch_msgs = 0;
      if ((rc = growDevice(h, &P->d_scratch, &a, applied.size() * 4 * h->dv.cols, true))) return rc;
      if ((rc = growDevice(h, &P->d_touched, &b, applied.size() * L->ly.tw, true))) return rc;
      P->scratch_msgs = applied.size();
    }
    HIP_TRY(waitStream(h->stream));  // (the staging block is free)
    memcpy(P->h_stage, applied.data(), o_leaves);
    if (!leaves.empty()) memcpy(P->h_stage + o_leaves, leaves.data(), sizeof(C3dBoxCells) * leaves.size());
    HIP_TRY(hipMemcpyAsync(P->d_stage, P->h_stage, bytes, hipMemcpyHostToDevice, h->stream));
    C3dCells c{};
    c.msgs = reinterpret_cast<const C3dCellsMsg*>(P->d_stage);
    c.leaves = reinterpret_cast<const C3dBoxCells*>(P->d_stage + o_leaves);
    c.scratch = P->d_scratch;
    c.touched = P->d_touched;
    c.n_msgs = (uint32_t)applied.size();
    c.n_leaves = (uint32_t)leaves.size();
    c.max_columns = max_columns;
    launch_c3d_cells(h->dv, L->ly, c, h->stream);
    if ((rc = checkLaunch())) return rc;
  }
  P->subs.swap(subs);
  P->subs_of = L;
  if (verdicts_out) std::copy(verdicts.begin(), verdicts.end(), verdicts_out);
  return NAVGPU_OK;  // queued
}

}  // extern "C"
