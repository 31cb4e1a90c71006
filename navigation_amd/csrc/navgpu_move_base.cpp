// move_base's planner-side executive for a fleet (include/navgpu.h, "move_base's planner-side executive"): polygon writes into
// the master / obstacle grid (Costmap2D::setConvexPolygonCost), MoveBase::clearCostmapWindows on top of them, the handover of a
// NavFn batch's plans to the controller with MoveBase::preferPrevPlan's persistence policy, and MoveBase::planService's goal search
// as batches of candidate plans.  move_base_kernels.hip has the kernels; the service runs the NavFn families' own.
#include "navgpu_navfn.h"

namespace {

using Robot = navgpu_fleet::ResidentPlans::Robot;

// the per-robot arrays of this file's calls: once (left in place by a call that fails later)
int reserveMoveBase(navgpu_fleet* f) {
  navgpu_fleet::MoveBaseState& mb = f->mb;
  const size_t n = f->desc.n_instances;
  int rc = NAVGPU_OK;
  if (!rc && !mb.d_persist) rc = f->alloc(&mb.d_persist, n);  // (zeroed: PERSISTENCE_INITIAL)
  if (!rc && !mb.d_in) rc = f->alloc(&mb.d_in, n);
  if (!rc && !mb.h_in) rc = f->allocPinned(&mb.h_in, n);
  if (!rc && !mb.d_rec) rc = f->alloc(&mb.d_rec, n);
  if (!rc && !mb.h_rec) rc = f->allocPinned(&mb.h_rec, n);
  if (!rc && !mb.d_poly_off) rc = f->alloc(&mb.d_poly_off, n + 1);
  if (!rc && !mb.h_poly_off) rc = f->allocPinned(&mb.h_poly_off, n + 1);
  if (!rc && !mb.d_poly_ok) rc = f->alloc(&mb.d_poly_ok, n);
  if (!rc && !mb.h_poly_ok) rc = f->allocPinned(&mb.h_poly_ok, n);
  return rc;
}

// the persistence states are written by handovers on the NavFn handle's stream and by the three calls below on the fleet's
int persistenceReady(navgpu_fleet* f) {
  if (!f->rp.cap) return NAVGPU_ERR_STATE;
  int rc = reserveMoveBase(f);
  if (rc) return rc;
  return waitAdoption(f);
}

int setPolygonCost(navgpu_fleet* f, int grid, uint32_t first, uint32_t count, const double* polys_xy, const uint32_t* offsets, uint8_t value,
                   int32_t* ok_out) {
  CostmapDev& cm = f->cm;
  uint8_t* base = nullptr;
  switch (grid) {
    case NAVGPU_GRID_MASTER: base = cm.master; break;
    case NAVGPU_GRID_OBSTACLE: base = cm.obst; break;  // (a VoxelLayer's 2-D grid too: setConvexPolygonCost is Costmap2D's)
    default: return NAVGPU_ERR_INVALID;
  }
  for (uint32_t k = 0; k < count; ++k)
    if (offsets[k + 1] < offsets[k]) return NAVGPU_ERR_INVALID;
  const uint32_t total = offsets[count] - offsets[0];
  if (total && !polys_xy) return NAVGPU_ERR_INVALID;
  if (!base) return NAVGPU_ERR_STATE;
  if (f->desc.rolling_window && f->shift_pending) return NAVGPU_ERR_STATE;  // the origins on the device are not the grids' yet
  for (uint32_t k = 0; k < count; ++k)
    if (offsets[k + 1] - offsets[k] > NAVGPU_MAX_POLYGON) {
      g_last_error = "navgpu_costmap_set_polygon_cost: polygon " + std::to_string(k) + " has more than NAVGPU_MAX_POLYGON vertices";
      return NAVGPU_ERR_CAPACITY;
    }
  navgpu_fleet::MoveBaseState& mb = f->mb;
  int rc = reserveMoveBase(f);
  if (rc) return rc;
  if (total > mb.poly_cap) {  // (the write before this one has been waited for)
    double* q = nullptr;
    if ((rc = f->alloc(&q, 2 * (size_t)total)) != NAVGPU_OK) return rc;
    f->release(mb.d_poly_xy);
    mb.d_poly_xy = q;
    mb.poly_cap = total;
  }
  for (uint32_t k = 0; k <= count; ++k) mb.h_poly_off[k] = offsets[k] - offsets[0];
  HIP_TRY(hipMemcpyAsync(mb.d_poly_off, mb.h_poly_off, sizeof(uint32_t) * (count + 1), hipMemcpyHostToDevice, f->stream));
  if (total)
    HIP_TRY(hipMemcpyAsync(mb.d_poly_xy, polys_xy + 2 * (size_t)offsets[0], sizeof(double) * 2 * total, hipMemcpyHostToDevice, f->stream));
  f->touchInputs(first, count);
  launch_set_polygon_cost(cm, base, first, count, mb.d_poly_xy, mb.d_poly_off, value, mb.d_poly_ok, f->stream);
  HIP_TRY(hipMemcpyAsync(mb.h_poly_ok, mb.d_poly_ok, sizeof(int32_t) * count, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));  // the caller's buffer and the staging arrays are free again
  if ((rc = checkLaunch()) != NAVGPU_OK) return rc;
  if (ok_out) memcpy(ok_out, mb.h_poly_ok, sizeof(int32_t) * count);
  return NAVGPU_OK;
}

// planService's candidate goals (move_base.cpp:372-396), the exact goal first.  The loop variables are floats as in the reference; every
// comparison and sum is spelled with the promotions C++ gives the reference's expressions.  Stops once `limit` candidates are exceeded.
void planServiceCandidates(double gx, double gy, double resolution_in, double tolerance, size_t limit, std::vector<double>& xy) {
  xy.clear();
  xy.push_back(gx);
  xy.push_back(gy);
  const float resolution = (float)resolution_in;
  float search_increment = resolution * 3.0;
  if (tolerance > 0.0 && tolerance < search_increment) search_increment = tolerance;
  if (!(search_increment > 0.0f)) return;  // (the reference's loops would not end)
  for (float max_offset = search_increment; max_offset <= tolerance; max_offset += search_increment)
    for (float y_offset = 0; y_offset <= max_offset; y_offset += search_increment)
      for (float x_offset = 0; x_offset <= max_offset; x_offset += search_increment) {
        if (x_offset < max_offset - 1e-9 && y_offset < max_offset - 1e-9) continue;  // not again inside the current outer layer
        for (float y_mult = -1.0; y_mult <= 1.0 + 1e-9; y_mult += 2.0) {
          if (y_offset < 1e-9 && y_mult < -1.0 + 1e-9) continue;  // -1 * 0 is still 0
          for (float x_mult = -1.0; x_mult <= 1.0 + 1e-9; x_mult += 2.0) {
            if (x_offset < 1e-9 && x_mult < -1.0 + 1e-9) continue;
            if (xy.size() / 2 > limit) return;
            const float dy = y_offset * y_mult, dx = x_offset * x_mult;
            xy.push_back(gx + dx);
            xy.push_back(gy + dy);
          }
        }
      }
}

}  // namespace

extern "C" {

int navgpu_move_base_plan_service_candidates(const double* goal_xy, double resolution, double tolerance, uint32_t capacity, double* out_xy) {
  if (!goal_xy || (capacity && !out_xy) || !(resolution > 0.0) || !std::isfinite(resolution)) return NAVGPU_ERR_INVALID;
  std::vector<double> xy;
  planServiceCandidates(goal_xy[0], goal_xy[1], resolution, tolerance, NAVGPU_PLAN_SERVICE_MAX_CANDIDATES, xy);
  const size_t n = xy.size() / 2;
  if (out_xy) memcpy(out_xy, xy.data(), sizeof(double) * 2 * std::min<size_t>(n, capacity));
  return (int)n;
}

int navgpu_move_base_plan_service(navgpu_navfn* h, uint32_t first_slot, uint32_t slots_per_request, uint32_t n_requests, int32_t family,
                                  const navgpu_global_planner_params* gp, const navgpu_make_plan_options* opt, const navgpu_navfn_ros_params* nr,
                                  const navgpu_plan_service_request* req, navgpu_plan_service_result* results, void* winner_results) {
  if (!h || !req || !results || !n_requests || !slots_per_request) return NAVGPU_ERR_INVALID;
  if ((uint64_t)n_requests * slots_per_request > 0xFFFFFFFFull || !navfnRange(h, first_slot, n_requests * slots_per_request)) return NAVGPU_ERR_INVALID;
  const bool is_gp = family == NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER;
  if (!is_gp && family != NAVGPU_PLAN_FAMILY_NAVFN_ROS) return NAVGPU_ERR_INVALID;
  if (is_gp ? (!gp || !opt) : !nr) return NAVGPU_ERR_INVALID;
  const uint32_t S = slots_per_request;
  std::vector<std::vector<double>> cand(n_requests);
  for (uint32_t q = 0; q < n_requests; ++q) {
    if (!(req[q].frame[2] > 0.0) || !std::isfinite(req[q].frame[2])) return NAVGPU_ERR_INVALID;
    planServiceCandidates(req[q].goal[0], req[q].goal[1], req[q].frame[2], req[q].tolerance, NAVGPU_PLAN_SERVICE_MAX_CANDIDATES, cand[q]);
    if (cand[q].size() / 2 > NAVGPU_PLAN_SERVICE_MAX_CANDIDATES) {
      g_last_error = "navgpu_move_base_plan_service: request " + std::to_string(q) + " has more than NAVGPU_PLAN_SERVICE_MAX_CANDIDATES candidates";
      return NAVGPU_ERR_INVALID;
    }
  }
  NavfnGuard guard_(h);
  const size_t res_bytes = is_gp ? sizeof(navgpu_make_plan_result) : sizeof(navgpu_navfn_ros_result);
  if (winner_results) memset(winner_results, 0, res_bytes * n_requests);
  std::vector<uint8_t> active(n_requests, 1);
  for (uint32_t q = 0; q < n_requests; ++q) results[q] = navgpu_plan_service_result{-1, -1, 0, (int32_t)(cand[q].size() / 2), 0, 0};
  std::vector<double> frames, starts, goals, tols;
  std::vector<navgpu_make_plan_result> gp_res;
  std::vector<navgpu_navfn_ros_result> nr_res;
  for (uint32_t round = 0;; ++round) {
    bool any = false;
    for (uint32_t q = 0; q < n_requests; ++q) {
      if (active[q] && (size_t)round * S >= cand[q].size() / 2) {  // every candidate failed
        active[q] = 0;
        results[q].tried = results[q].n_candidates;
      }
      any = any || active[q];
    }
    if (!any) break;
    for (uint32_t q0 = 0; q0 < n_requests;) {  // one batch per run of requests that are still searching
      if (!active[q0]) {
        ++q0;
        continue;
      }
      uint32_t q1 = q0;
      while (q1 < n_requests && active[q1]) ++q1;
      const uint32_t count = (q1 - q0) * S;
      frames.resize(3 * (size_t)count);
      starts.resize(3 * (size_t)count);
      goals.resize(3 * (size_t)count);
      tols.resize(count);
      for (uint32_t q = q0; q < q1; ++q) {
        const size_t nc = cand[q].size() / 2;
        for (uint32_t j = 0; j < S; ++j) {
          // a slot behind the request's last candidate repeats it (its result is not read)
          const size_t c = std::min((size_t)round * S + j, nc - 1), at = (size_t)(q - q0) * S + j;
          memcpy(&frames[3 * at], req[q].frame, sizeof(double) * 3);
          memcpy(&starts[3 * at], req[q].start, sizeof(double) * 3);
          goals[3 * at] = cand[q][2 * c];
          goals[3 * at + 1] = cand[q][2 * c + 1];
          goals[3 * at + 2] = req[q].goal[2];
          tols[at] = req[q].default_tolerance;
        }
      }
      const uint32_t first = first_slot + q0 * S;
      int rc;
      if (is_gp) {
        gp_res.resize(count);
        rc = navgpu_global_planner_make_plan(h, first, count, gp, opt, frames.data(), starts.data(), goals.data(), gp_res.data());
      } else {
        nr_res.resize(count);
        rc = navgpu_navfn_ros_make_plan(h, first, count, nr, frames.data(), starts.data(), goals.data(), tols.data(), nr_res.data());
      }
      if (rc) return rc;  // (in the first round: nothing has run)
      for (uint32_t q = q0; q < q1; ++q) {
        const size_t nc = cand[q].size() / 2;
        ++results[q].rounds;
        for (uint32_t j = 0; j < S && (size_t)round * S + j < nc; ++j) {
          const size_t at = (size_t)(q - q0) * S + j;
          const int32_t status = is_gp ? gp_res[at].status : nr_res[at].status, np = is_gp ? gp_res[at].n_poses : nr_res[at].n_poses;
          if (status != NAVGPU_MAKE_PLAN_OK || np <= 0) continue;
          const uint32_t slot = first + (uint32_t)at;
          navgpu_plan_service_result& r = results[q];
          r.winner = (int32_t)(round * S + j);
          r.slot = (int32_t)slot;
          r.tried = r.winner + 1;
          r.n_poses = np;
          if (r.winner > 0) {  // global_plan.push_back(req.goal) (:402): the plan's record gains a tail pose for the emit pass
            navgpu::GpPlanRec& rec = h->made.rec[slot];
            rec.has_tail = 1;
            rec.n_poses = np + 1;
            rec.tail_x = req[q].goal[0];
            rec.tail_y = req[q].goal[1];
            rec.tail_yaw = req[q].goal[2];
            HIP_TRY(hipMemcpyAsync(h->made.d_rec + slot, &rec, sizeof(rec), hipMemcpyHostToDevice, h->stream));
            r.n_poses = np + 1;
          }
          if (winner_results)
            memcpy((uint8_t*)winner_results + res_bytes * q, is_gp ? (const void*)&gp_res[at] : (const void*)&nr_res[at], res_bytes);
          active[q] = 0;
          break;
        }
      }
      q0 = q1;
    }
    HIP_TRY(waitStream(h->stream));  // the records' copies have run
  }
  return NAVGPU_OK;
}

int navgpu_costmap_set_polygon_cost(navgpu_fleet* f, int grid, uint32_t first, uint32_t count, const double* polys_xy, const uint32_t* offsets,
                                    uint8_t value, int32_t* ok_out) {
  if (!f || !offsets || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  return setPolygonCost(f, grid, first, count, polys_xy, offsets, value, ok_out);
}

int navgpu_move_base_clear_costmap_windows(navgpu_fleet* f, uint32_t first, uint32_t count, const double* poses_xy, double size_x, double size_y,
                                           int32_t* ok_out) {
  if (!f || !poses_xy || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  std::vector<double> poly((size_t)count * 8);
  std::vector<uint32_t> off(count + 1);
  for (uint32_t k = 0; k < count; ++k) {  // move_base.cpp:284-302
    const double x = poses_xy[2 * k], y = poses_xy[2 * k + 1];
    double* pt = &poly[(size_t)k * 8];
    pt[0] = x - size_x / 2;
    pt[1] = y - size_y / 2;
    pt[2] = x + size_x / 2;
    pt[3] = y - size_y / 2;
    pt[4] = x + size_x / 2;
    pt[5] = y + size_y / 2;
    pt[6] = x - size_x / 2;
    pt[7] = y + size_y / 2;
    off[k] = 4 * k;
  }
  off[count] = 4 * count;
  return setPolygonCost(f, NAVGPU_GRID_MASTER, first, count, poly.data(), off.data(), kFree, ok_out);
}

int navgpu_move_base_handover_plans(navgpu_fleet* f, uint32_t fleet_first, navgpu_navfn* h, uint32_t nav_first, uint32_t count, int32_t family,
                                    const double* T, const double* positions_xy, int64_t now_ns, int64_t persistence_timeout_ns,
                                    navgpu_handover_record* out) {
  if (!f || !h || !positions_xy || persistence_timeout_ns < 0 || !f->rangeOk(fleet_first, count) || !navfnRange(h, nav_first, count))
    return NAVGPU_ERR_INVALID;
  if (family != NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER && family != NAVGPU_PLAN_FAMILY_NAVFN_ROS) return NAVGPU_ERR_INVALID;
  if (f->desc.device != h->device) return NAVGPU_ERR_INVALID;
  NavfnGuard nav_guard_(h);  // (the order of navgpu_local_planner_adopt_plans)
  FleetGuard guard_(f);
  navgpu_fleet::ResidentPlans& rp = f->rp;
  if (!rp.cap || !f->lp_configured || !f->planner_configured) return NAVGPU_ERR_STATE;
  const uint8_t maker = family == NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER ? kMadeByGlobalPlanner : kMadeByNavfnRos;
  MadePlans& m = h->made;
  for (uint32_t k = 0; k < count; ++k)
    if (m.valid.empty() || m.valid[nav_first + k] != maker) {
      g_last_error = "navgpu_move_base_handover_plans: a plan of the range was not made by the last make_plan call of that family";
      return NAVGPU_ERR_STATE;
    }
  navgpu_fleet::MoveBaseState& mb = f->mb;
  int rc = persistenceReady(f);
  if (rc) return rc;
  bool any = false, too_long = false;
  std::vector<uint8_t> cand(count, 0);
  for (uint32_t k = 0; k < count; ++k) {
    const int32_t np = m.rec[nav_first + k].n_poses;
    const Robot& R = rp.robots[fleet_first + k];
    const bool res = rp.residentAt(fleet_first + k);
    cand[k] = np > 0 && (uint32_t)np <= rp.cap;
    any = any || cand[k];
    PlanPreferIn& a = mb.h_in[k];  // (the copy out of it has run: the handover before this one waited for its records)
    a = PlanPreferIn{};
    a.x = positions_xy[2 * k];
    a.y = positions_xy[2 * k + 1];
    a.stored = res ? R.start + R.len : 0;
    a.dropped = res ? R.dropped : 0;
    a.new_len = np > 0 ? (uint32_t)np : 0;
    a.flags = cand[k] ? kPpActive : 0u;
    navgpu_handover_record& r = mb.h_rec[k];  // what the kernel leaves alone: a plan that was not made, or is too long
    r = navgpu_handover_record{};
    r.new_len = (int32_t)a.new_len;
    r.dropped = (int32_t)a.dropped;
    if (np > 0 && (uint32_t)np > rp.cap) {
      too_long = true;
      r.decision = NAVGPU_HANDOVER_TOO_LONG;
    }
  }
  // The NavFn stream reads and writes the slots once the fleet's stream has finished with them, and the fleet's stream goes on once
  // they are written: two events, no device-wide wait.  The decision kernel, the emit kernel it predicates and the records' copy
  // are queued back to back; the host sees the decisions only afterwards.
  HIP_TRY(hipEventRecord(rp.ev_fleet, f->stream));
  HIP_TRY(hipStreamWaitEvent(h->stream, rp.ev_fleet, 0));
  if (any) {
    HIP_TRY(hipMemcpyAsync(mb.d_in, mb.h_in, sizeof(PlanPreferIn) * count, hipMemcpyHostToDevice, h->stream));
    launch_plan_prefer(rp.d_poses, rp.cap, fleet_first, count, mb.d_in, mb.d_persist, now_ns, persistence_timeout_ns, mb.d_rec, rp.d_off, h->stream);
    const uint32_t capacity = f->desc.n_instances * rp.cap;
    for (uint32_t k = 0; k < count;) {
      if (!cand[k]) {
        ++k;
        continue;
      }
      uint32_t e = k;
      while (e < count && cand[e]) ++e;
      launch_gp_plan_emit(h->nv, nav_first + k, e - k, m.d_rec + nav_first + k, rp.d_off + k, rp.d_poses, capacity, h->stream);
      HIP_TRY(hipMemcpyAsync(mb.h_rec + k, mb.d_rec + k, sizeof(navgpu_handover_record) * (e - k), hipMemcpyDeviceToHost, h->stream));
      k = e;
    }
    if ((rc = checkLaunch()) != NAVGPU_OK) return rc;
  }
  // the states of the robots left alone, for their records
  for (uint32_t k = 0; k < count; ++k)
    if (!cand[k])
      HIP_TRY(hipMemcpyAsync(&mb.h_rec[k].persistence_end_ns, mb.d_persist + fleet_first + k, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipEventRecord(rp.ev_nav, h->stream));
  rp.ev_nav_set = true;
  HIP_TRY(hipStreamWaitEvent(f->stream, rp.ev_nav, 0));
  HIP_TRY(waitStream(h->stream));
  if (out) memcpy(out, mb.h_rec, sizeof(navgpu_handover_record) * count);
  for (uint32_t k = 0; k < count;) {  // DWAPlannerROS::setPlan's host side for the robots that took their plan
    if (mb.h_rec[k].decision != NAVGPU_HANDOVER_ADOPT) {
      ++k;
      continue;
    }
    uint32_t e = k;
    while (e < count && mb.h_rec[e].decision == NAVGPU_HANDOVER_ADOPT) {
      becomeResident(f, fleet_first + e, (uint32_t)m.rec[nav_first + e].n_poses, T ? T + 3 * (size_t)e : nullptr);
      ++e;
    }
    if ((rc = navgpu_planner_set_plan(f, fleet_first + k, e - k)) != NAVGPU_OK) return rc;
    k = e;
  }
  if (too_long) {
    g_last_error = "navgpu_move_base_handover_plans: a plan is longer than max_global_plan and was not handed over";
    return NAVGPU_ERR_CAPACITY;
  }
  return NAVGPU_OK;
}

int navgpu_move_base_reset_persistence(navgpu_fleet* f, uint32_t first, uint32_t count) {
  if (!f || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  const int rc = persistenceReady(f);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(f->mb.d_persist + first, 0, sizeof(int64_t) * count, f->stream));  // PERSISTENCE_INITIAL
  return NAVGPU_OK;
}

int navgpu_move_base_get_persistence(navgpu_fleet* f, uint32_t first, uint32_t count, int64_t* persistence_end_ns) {
  if (!f || !persistence_end_ns || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  const int rc = persistenceReady(f);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(persistence_end_ns, f->mb.d_persist + first, sizeof(int64_t) * count, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  return NAVGPU_OK;
}

int navgpu_move_base_set_persistence(navgpu_fleet* f, uint32_t first, uint32_t count, const int64_t* persistence_end_ns) {
  if (!f || !persistence_end_ns || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  const int rc = persistenceReady(f);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(f->mb.d_persist + first, persistence_end_ns, sizeof(int64_t) * count, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(waitStream(f->stream));  // the caller's buffer is free again
  return NAVGPU_OK;
}

}  // extern "C"
