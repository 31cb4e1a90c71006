// navgpu_costmap3d_*: host side of the batched Costmap3DQuery (costmap3d_kernels.hip, include/navgpu.h).
// Every argument check runs before the device is opened (openDevice) and before anything is queued.
#include <cfloat>
#include <cmath>
#include <map>

#include "navgpu_costmap3d.h"
#include "navgpu_fleet.h"

struct navgpu_costmap3d {
  navgpu_costmap3d_desc desc{};
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
    hipStreamDestroy(h->stream);
  }
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
