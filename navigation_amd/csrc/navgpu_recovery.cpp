// C-ABI host side of the batched footprint-cost query and the two behaviours built on it (include/navgpu.h):
//   navgpu_footprint_cost            WorldModel::footprintCost -> CostmapModel::footprintCost, called directly
//   navgpu_rotate_recovery_*         rotate_recovery::RotateRecovery::runBehavior, one loop pass per call
//   navgpu_carrot_plan               carrot_planner::CarrotPlanner::makePlan's search
// The host builds the query poses - sums and products of doubles in the reference's order, so they are the reference's
// doubles - and reads back one index per robot; every footprint is laid down by k_footprint_cost (footprint_kernels.hip).
#include "navgpu_fleet.h"

namespace {

double normalizeAngle(double a) { return navgpu_shortest_angular_distance(0.0, a); }  // angles::normalize_angle, fmod form

// Room for `total` queries in the staging buffers.  All-or-nothing: the fleet keeps its buffers when an allocation fails.
int reserveQueries(navgpu_fleet* f, uint32_t total) {
  navgpu_fleet::FootprintQueries& q = f->fq;
  const uint32_t n = f->desc.n_instances;
  int rc;
  if (!q.d_off) {
    navgpu_fleet::FootprintQueries t;
    if ((rc = f->alloc(&t.d_off, (size_t)n + 1)) == NAVGPU_OK && (rc = f->alloc(&t.d_first, n)) == NAVGPU_OK &&
        (rc = f->allocPinned(&t.h_off, (size_t)n + 1)) == NAVGPU_OK)
      rc = f->allocPinned(&t.h_first, n);
    if (rc != NAVGPU_OK) {
      f->release(t.d_off);
      f->release(t.d_first);
      f->releasePinned(t.h_off);
      f->releasePinned(t.h_first);
      return rc;
    }
    q.d_off = t.d_off;
    q.d_first = t.d_first;
    q.h_off = t.h_off;
    q.h_first = t.h_first;
  }
  if (total <= q.cap) return NAVGPU_OK;
  uint32_t cap = std::max<uint32_t>(q.cap, 4096);
  while (cap < total) cap *= 2;
  double *d_poses = nullptr, *d_costs = nullptr, *h_poses = nullptr, *h_costs = nullptr;
  if ((rc = f->alloc(&d_poses, (size_t)cap * 3)) == NAVGPU_OK && (rc = f->alloc(&d_costs, cap)) == NAVGPU_OK &&
      (rc = f->allocPinned(&h_poses, (size_t)cap * 3)) == NAVGPU_OK)
    rc = f->allocPinned(&h_costs, cap);
  hipError_t e = rc == NAVGPU_OK ? waitStream(f->stream) : hipSuccess;  // (the fresh buffers' memsets; nothing queued reads the old ones)
  if (rc == NAVGPU_OK && e != hipSuccess) {
    g_last_error = std::string("footprint queries: ") + hipGetErrorString(e);
    rc = NAVGPU_ERR_HIP;
  }
  if (rc != NAVGPU_OK) {
    f->release(d_poses);
    f->release(d_costs);
    f->releasePinned(h_poses);
    f->releasePinned(h_costs);
    return rc;
  }
  f->release(q.d_poses);
  f->release(q.d_costs);
  f->releasePinned(q.h_poses);
  f->releasePinned(q.h_costs);
  q.d_poses = d_poses;
  q.d_costs = d_costs;
  q.h_poses = h_poses;
  q.h_costs = h_costs;
  q.cap = cap;
  return NAVGPU_OK;
}

// prefix sums of the run lengths into fq.h_off (reserving room); NAVGPU_ERR_CAPACITY beyond 2^28 queries
int stageRuns(navgpu_fleet* f, uint32_t count, const uint32_t* counts) {
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; ++k) total += counts[k];
  if (total > (1ull << 28)) return NAVGPU_ERR_CAPACITY;
  int rc = reserveQueries(f, (uint32_t)total);
  if (rc) return rc;
  uint32_t at = 0;
  for (uint32_t k = 0; k < count; ++k) {
    f->fq.h_off[k] = at;
    at += counts[k];
  }
  f->fq.h_off[count] = at;
  return NAVGPU_OK;
}

// The staged queries (fq.h_off, fq.h_poses) through k_footprint_cost, behind whatever the stream holds; on return
// fq.h_first (and fq.h_costs when asked for) hold the results.
int runQueries(navgpu_fleet* f, uint32_t first, uint32_t count, const uint32_t* counts, int32_t allow_unknown, int32_t seek_legal, bool want_costs) {
  navgpu_fleet::FootprintQueries& q = f->fq;
  const uint32_t total = q.h_off[count];
  HIP_TRY(hipMemcpyAsync(q.d_off, q.h_off, sizeof(uint32_t) * ((size_t)count + 1), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemsetAsync(q.d_first, 0xFF, sizeof(uint32_t) * count, f->stream));
  if (total) {
    HIP_TRY(hipMemcpyAsync(q.d_poses, q.h_poses, sizeof(double) * 3 * (size_t)total, hipMemcpyHostToDevice, f->stream));
    FootprintDev d{};
    d.nx = f->cm.nx;
    d.ny = f->cm.ny;
    d.cells_padded = f->cm.cells_padded;
    d.res = f->cm.res;
    d.origin = f->cm.origin;
    d.master = f->cm.master;
    d.fp_spec = f->pl.fp_spec;
    d.fp_n = f->pl.fp_n;
    d.q_off = q.d_off;
    d.poses = q.d_poses;
    d.costs = q.d_costs;
    d.first_hit = q.d_first;
    d.allow_unknown = allow_unknown != 0;
    d.seek_legal = seek_legal != 0;
    PROFILED(f, NAVGPU_K_FOOTPRINT, launch_footprint_cost(d, first, count, counts, f->h_fp_n.data(), f->stream));
    int rc = checkLaunch();
    if (rc) return rc;
    if (want_costs) HIP_TRY(hipMemcpyAsync(q.h_costs, q.d_costs, sizeof(double) * total, hipMemcpyDeviceToHost, f->stream));
  }
  HIP_TRY(hipMemcpyAsync(q.h_first, q.d_first, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  return NAVGPU_OK;
}

bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
// the grids lag the origins between a rolling-window stage and its update
bool originsStale(const navgpu_fleet* f) { return f->desc.rolling_window && f->shift_pending; }

}  // namespace

extern "C" {

int navgpu_footprint_cost(navgpu_fleet* f, uint32_t first, uint32_t count, const uint32_t* counts, const double* poses, int32_t allow_unknown,
                          double* costs_out, int32_t* first_illegal_out) {
  if (!f || !counts || !f->rangeOk(first, count) || count > 65535) return NAVGPU_ERR_INVALID;
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; ++k) total += counts[k];
  if (total && (!poses || !costs_out)) return NAVGPU_ERR_INVALID;
  for (uint64_t i = 0; i < total; ++i)
    if (!finite3(poses + 3 * i)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (originsStale(f)) return NAVGPU_ERR_STATE;
  int rc = stageRuns(f, count, counts);
  if (rc) return rc;
  if (total) memcpy(f->fq.h_poses, poses, sizeof(double) * 3 * (size_t)total);
  if ((rc = runQueries(f, first, count, counts, allow_unknown, 0, true))) return rc;
  if (total) memcpy(costs_out, f->fq.h_costs, sizeof(double) * (size_t)total);
  if (first_illegal_out) memcpy(first_illegal_out, f->fq.h_first, sizeof(int32_t) * count);  // 0xFFFFFFFF = -1: none
  return NAVGPU_OK;
}

int navgpu_rotate_recovery_configure(navgpu_fleet* f, const navgpu_rotate_recovery_params* p) {
  if (!f || !p) return NAVGPU_ERR_INVALID;
  if (!(p->sim_granularity > 0) || !std::isfinite(p->sim_granularity) || !std::isfinite(p->acc_lim_th) || !std::isfinite(p->max_rotational_vel) ||
      !std::isfinite(p->min_in_place_rotational_vel) || !std::isfinite(p->yaw_goal_tolerance))
    return NAVGPU_ERR_INVALID;
  if (2.0 * M_PI / p->sim_granularity > (double)(NAVGPU_ROTATE_RECOVERY_MAX_SWEEP - 1)) {
    g_last_error = "navgpu_rotate_recovery_configure: sim_granularity makes a sweep longer than NAVGPU_ROTATE_RECOVERY_MAX_SWEEP headings";
    return NAVGPU_ERR_CAPACITY;
  }
  FleetGuard guard_(f);
  f->rot = *p;
  return NAVGPU_OK;
}

int navgpu_rotate_recovery_step(navgpu_fleet* f, uint32_t first, uint32_t count, const double* poses, navgpu_rotate_recovery_state* state,
                                double* cmd_wz, int32_t* status) {
  if (!f || !poses || !state || !cmd_wz || !status || !f->rangeOk(first, count) || count > 65535) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k)
    if (!finite3(poses + 3 * k)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (originsStale(f)) return NAVGPU_ERR_STATE;
  const navgpu_rotate_recovery_params& P = f->rot;
  std::vector<navgpu_rotate_recovery_state> st(state, state + count);  // committed when nothing can fail any more
  std::vector<double> current(count), dist(count);
  std::vector<uint32_t> counts(count);
  for (uint32_t k = 0; k < count; ++k) {
    const double yaw = poses[3 * k + 2];
    if (!st[k].started) {  // :100-104
      st[k].start_offset = 0 - normalizeAngle(yaw);
      st[k].got_180 = 0;
      st[k].started = 1;
    }
    const double norm_angle = normalizeAngle(yaw);  // :108-112
    current[k] = normalizeAngle(norm_angle + st[k].start_offset);
    dist[k] = M_PI - current[k];
    uint32_t n = 0;
    for (double sim_angle = 0.0; sim_angle < dist[k]; sim_angle += P.sim_granularity)  // :117-129, the same repeated addition
      if (++n > NAVGPU_ROTATE_RECOVERY_MAX_SWEEP) return NAVGPU_ERR_CAPACITY;
    counts[k] = n;
  }
  int rc = stageRuns(f, count, counts.data());
  if (rc) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    double* q = f->fq.h_poses + (size_t)f->fq.h_off[k] * 3;
    double sim_angle = 0.0;
    for (uint32_t i = 0; i < counts[k]; ++i, sim_angle += P.sim_granularity) {
      q[3 * i] = poses[3 * k];
      q[3 * i + 1] = poses[3 * k + 1];
      q[3 * i + 2] = poses[3 * k + 2] + sim_angle;  // :119
    }
  }
  if ((rc = runQueries(f, first, count, counts.data(), P.allow_unknown, 0, false))) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    const int32_t illegal = (int32_t)f->fq.h_first[k];
    if (illegal >= 0) {  // :123-126
      st[k].swept = illegal + 1;
      st[k].started = 0;
      cmd_wz[k] = 0.0;
      status[k] = NAVGPU_ROTATE_BLOCKED;
      continue;
    }
    st[k].swept = (int32_t)counts[k];
    double vel = sqrt(2 * P.acc_lim_th * dist[k]);  // :131-135
    vel = std::min(std::max(vel, P.min_in_place_rotational_vel), P.max_rotational_vel);
    cmd_wz[k] = vel;
    if (current[k] < 0.0) st[k].got_180 = 1;  // :144-150
    if (st[k].got_180 && current[k] >= (0.0 - P.yaw_goal_tolerance)) {
      st[k].started = 0;
      status[k] = NAVGPU_ROTATE_DONE;
    } else {
      status[k] = NAVGPU_ROTATE_RUNNING;
    }
  }
  std::copy(st.begin(), st.end(), state);
  return NAVGPU_OK;
}

int navgpu_carrot_plan(navgpu_fleet* f, uint32_t first, uint32_t count, const double* starts, const double* goals, int32_t allow_unknown,
                       double* targets, int32_t* found) {
  if (!f || !starts || !goals || !targets || !found || !f->rangeOk(first, count) || count > 65535) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k)
    if (!finite3(starts + 3 * k) || !finite3(goals + 3 * k)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (originsStale(f)) return NAVGPU_ERR_STATE;
  std::vector<double> scales;  // :131-153: the same for every plan
  for (double scale = 1.0; !(scale < 0); scale -= 0.01) scales.push_back(scale);
  std::vector<uint32_t> counts(count);
  for (uint32_t k = 0; k < count; ++k) counts[k] = f->h_fp_n[first + k] < 3 ? 0u : (uint32_t)scales.size();  // :76-79
  int rc = stageRuns(f, count, counts.data());
  if (rc) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    double* q = f->fq.h_poses + (size_t)f->fq.h_off[k] * 3;
    const double start_x = starts[3 * k], start_y = starts[3 * k + 1], start_yaw = starts[3 * k + 2];
    const double diff_x = goals[3 * k] - start_x, diff_y = goals[3 * k + 1] - start_y;  // :122-124
    const double diff_yaw = normalizeAngle(goals[3 * k + 2] - start_yaw);
    for (uint32_t i = 0; i < counts[k]; ++i) {  // :144-146
      q[3 * i] = start_x + scales[i] * diff_x;
      q[3 * i + 1] = start_y + scales[i] * diff_y;
      q[3 * i + 2] = normalizeAngle(start_yaw + scales[i] * diff_yaw);
    }
  }
  if ((rc = runQueries(f, first, count, counts.data(), allow_unknown, 1, false))) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    const int32_t legal = (int32_t)f->fq.h_first[k];
    const double* t = legal >= 0 ? f->fq.h_poses + ((size_t)f->fq.h_off[k] + legal) * 3 : starts + 3 * k;  // :136-143
    targets[3 * k] = t[0];
    targets[3 * k + 1] = t[1];
    targets[3 * k + 2] = t[2];
    found[k] = legal >= 0 ? legal + 1 : 0;
  }
  return NAVGPU_OK;
}

}  // extern "C"
