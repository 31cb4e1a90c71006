// Device-resident global plans (include/navgpu.h, "Device-resident global plans"): the store, its batched setPlan, the adoption
// of a NavFn batch's plans without a read-back, and what the control cycle (navgpu_local_planner.cpp) calls through
// navgpu_fleet::ResidentPlans' function pointers - k_plan_window's launch and read-back, getGoalPose, the stored plan.
// local_plan_kernels.hip has the kernels.
#include "navgpu_navfn.h"

using Robot = navgpu_fleet::ResidentPlans::Robot;

namespace navgpu {

// the slot offsets / plan offsets in h_off may still feed an adoption's copy on the NavFn handle's stream
int waitAdoption(navgpu_fleet* f) {
  if (f->rp.ev_nav_set) HIP_TRY(hipEventSynchronize(f->rp.ev_nav));
  f->rp.ev_nav_set = false;
  return NAVGPU_OK;
}

// a robot's plan has been replaced: DWAPlannerROS::setPlan's host side (latch cleared), the host copy dropped
void becomeResident(navgpu_fleet* f, uint32_t i, uint32_t len, const double* T) {
  Robot& R = f->rp.robots[i];
  R.resident = true;
  R.start = 0;
  R.dropped = 0;
  R.len = len;
  R.has_T = T != nullptr;
  if (T) memcpy(R.T, T, sizeof(R.T));
  R.goal_known = false;
  R.loc_first = R.loc_n = 0;
  navgpu_fleet::LocalPlannerState& st = f->lp[i];
  st.xy_tolerance_latch = false;  // latchedStopRotateController_.resetLatching() (dwa_planner_ros.cpp:136)
  st.plan.clear();
  st.have_plan = false;
  st.local.clear();
  st.window = navgpu_local_window{-1, 0, 0, 0, (int32_t)len, NAVGPU_LOCAL_WINDOW_NONE};
}

}  // namespace navgpu

namespace {

void toGlobal(const Robot& R, const navgpu_global_pose& p, double out[3]) {  // goal_functions.cpp:148-150, planar
  if (R.has_T) {
    const double c = cos(R.T[2]), sn = sin(R.T[2]);
    out[0] = c * p.x - sn * p.y + R.T[0];
    out[1] = sn * p.x + c * p.y + R.T[1];
    out[2] = p.yaw + R.T[2];
  } else {
    out[0] = p.x;
    out[1] = p.y;
    out[2] = p.yaw;
  }
}

int windowPass(navgpu_fleet* f, uint32_t first, uint32_t count, const navgpu_robot_input* in, double dist_threshold) {
  navgpu_fleet::ResidentPlans& rp = f->rp;
  bool any = false;
  for (uint32_t k = 0; k < count; ++k) {
    const Robot& R = rp.robots[first + k];
    PlanWindowIn& a = rp.h_in[first + k];  // (the copy out of it has run: the pass before this one waited for its records)
    a = PlanWindowIn{};
    if (!R.resident || !in[k].have_pose || R.len == 0) continue;
    any = true;
    a.flags = kPwActive | (f->lp_lim[first + k].prune_plan ? kPwPrune : 0u);  // LocalPlannerLimits::prune_plan of this robot
    a.pose[0] = in[k].pose[0];
    a.pose[1] = in[k].pose[1];
    a.robot[0] = in[k].pose[0];
    a.robot[1] = in[k].pose[1];
    a.c = 1.0;
    if (R.has_T) {  // the robot in the frame of the plan, as navgpu_local_plan_window takes it
      a.flags |= kPwTransform;
      a.c = cos(R.T[2]);
      a.sn = sin(R.T[2]);
      const double dx = in[k].pose[0] - R.T[0], dy = in[k].pose[1] - R.T[1];
      a.robot[0] = a.c * dx + a.sn * dy;
      a.robot[1] = -a.sn * dx + a.c * dy;
      a.tx = R.T[0];
      a.ty = R.T[1];
      a.tyaw = R.T[2];
    }
    a.start = R.start;
    a.len = R.len;
  }
  if (!any) return NAVGPU_OK;
  HIP_TRY(hipMemcpyAsync(rp.d_in + first, rp.h_in + first, sizeof(PlanWindowIn) * count, hipMemcpyHostToDevice, f->stream));
  launch_plan_window(f->pl, rp.d_poses, rp.cap, first, count, rp.d_in, rp.d_rec, dist_threshold * dist_threshold, f->stream);
  HIP_TRY(hipMemcpyAsync(rp.h_rec + first, rp.d_rec + first, sizeof(PlanWindowRec) * count, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  return checkLaunch();
}

bool goalPose(navgpu_fleet* f, uint32_t i, double goal[3]) {
  navgpu_fleet::ResidentPlans& rp = f->rp;
  Robot& R = rp.robots[i];
  if (R.len == 0) return false;
  if (!R.goal_known) {  // (an adopted plan before its first cycle: the host has not seen its last pose)
    navgpu_global_pose g;
    if (hipMemcpyAsync(&g, rp.d_poses + (size_t)i * rp.cap + R.start + R.len - 1, sizeof(g), hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        waitStream(f->stream) != hipSuccess) {
      g_last_error = "resident plan: reading the goal pose failed";
      return false;
    }
    toGlobal(R, g, R.goal);
    R.goal_known = true;
  }
  memcpy(goal, R.goal, sizeof(R.goal));
  return true;
}

int readSlot(navgpu_fleet* f, uint32_t i, uint32_t at, uint32_t n, double* xyyaw) {
  if (!n) return NAVGPU_OK;
  HIP_TRY(hipMemcpyAsync(xyyaw, f->rp.d_poses + (size_t)i * f->rp.cap + at, sizeof(navgpu_global_pose) * n, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  return NAVGPU_OK;
}

int storedPlan(navgpu_fleet* f, uint32_t i, double* xyyaw, uint32_t capacity) {
  const Robot& R = f->rp.robots[i];
  if (xyyaw) {
    if (capacity < R.len) return NAVGPU_ERR_CAPACITY;
    const int rc = readSlot(f, i, R.start, R.len, xyyaw);
    if (rc) return rc;
  }
  return (int)R.len;
}

}  // namespace

extern "C" {

int navgpu_local_planner_reserve_plans(navgpu_fleet* f, uint32_t max_global_plan) {
  if (!f || !max_global_plan) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  navgpu_fleet::ResidentPlans& rp = f->rp;
  const uint32_t n = f->desc.n_instances;
  // slots are addressed with 32-bit pose offsets, and k_plan_window indexes a plan with ints
  if ((uint64_t)n * max_global_plan > 0xFFFFFFFFull || max_global_plan > 0x7FFFFFFFu) return NAVGPU_ERR_CAPACITY;
  if (rp.robots.size() != n) rp.robots.assign(n, Robot());
  for (uint32_t i = 0; i < n; ++i)
    if (rp.residentAt(i) && rp.robots[i].len > max_global_plan) {
      g_last_error = "navgpu_local_planner_reserve_plans: the resident plan of instance " + std::to_string(i) + " is longer than the new size";
      return NAVGPU_ERR_CAPACITY;
    }
  // what does not depend on the size: once (left in place by a call that fails later - the store stays absent)
  int rc = NAVGPU_OK;
  if (!rc && !rp.d_in) rc = f->alloc(&rp.d_in, n);
  if (!rc && !rp.h_in) rc = f->allocPinned(&rp.h_in, n);
  if (!rc && !rp.d_rec) rc = f->alloc(&rp.d_rec, n);
  if (!rc && !rp.h_rec) rc = f->allocPinned(&rp.h_rec, n);
  if (!rc && !rp.d_off) rc = f->alloc(&rp.d_off, (size_t)n + 1);
  if (!rc && !rp.h_off) rc = f->allocPinned(&rp.h_off, (size_t)n + 1);
  if (rc) return rc;
  if (!rp.ev_fleet) HIP_TRY(hipEventCreateWithFlags(&rp.ev_fleet, hipEventDisableTiming));
  if (!rp.ev_nav) HIP_TRY(hipEventCreateWithFlags(&rp.ev_nav, hipEventDisableTiming));
  // All-or-nothing, as navgpu_planner_configure: the new slots are allocated and filled on the side, and only when nothing can fail
  // any more is the old store released.
  navgpu_global_pose* np = nullptr;
  if ((rc = f->alloc(&np, (size_t)n * max_global_plan)) != NAVGPU_OK) return rc;
  hipError_t e = hipSuccess;
  for (uint32_t i = 0; i < n && e == hipSuccess; ++i) {
    const Robot& R = rp.robots[i];
    if (!rp.residentAt(i) || !R.len) continue;
    e = hipMemcpyAsync(np + (size_t)i * max_global_plan, rp.d_poses + (size_t)i * rp.cap + R.start, sizeof(navgpu_global_pose) * R.len,
                       hipMemcpyDeviceToDevice, f->stream);
  }
  if (e == hipSuccess) e = waitStream(f->stream);  // (also the allocation's memset, and whatever still read the old slots)
  if (e != hipSuccess) {
    g_last_error = std::string("navgpu_local_planner_reserve_plans: ") + hipGetErrorString(e);
    f->release(np);
    return NAVGPU_ERR_HIP;
  }
  // ---- commit
  for (uint32_t i = 0; i < n; ++i) {
    Robot& R = rp.robots[i];
    if (R.loc_n) R.loc_first -= R.start;
    R.dropped += R.start;  // the erased prefix is not carried over (navgpu_move_base_handover_plans reports it)
    R.start = 0;
  }
  f->release(rp.d_poses);
  rp.d_poses = np;
  rp.cap = max_global_plan;
  rp.window_pass = windowPass;
  rp.goal_pose = goalPose;
  rp.stored_plan = storedPlan;
  return NAVGPU_OK;
}

int navgpu_local_planner_set_plans(navgpu_fleet* f, uint32_t first, uint32_t count, const double* poses_xyyaw, const uint32_t* offsets,
                                   const double* T) {
  if (!f || !offsets || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k)
    if (offsets[k + 1] < offsets[k]) return NAVGPU_ERR_INVALID;
  const uint32_t total = offsets[count] - offsets[0];
  if (total && !poses_xyyaw) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  navgpu_fleet::ResidentPlans& rp = f->rp;
  if (!rp.cap || !f->lp_configured || !f->planner_configured) return NAVGPU_ERR_STATE;
  for (uint32_t k = 0; k < count; ++k)
    if (offsets[k + 1] - offsets[k] > rp.cap) {
      g_last_error = "navgpu_local_planner_set_plans: plan " + std::to_string(k) + " is longer than max_global_plan";
      return NAVGPU_ERR_CAPACITY;
    }
  int rc = waitAdoption(f);
  if (rc) return rc;
  const size_t bytes = sizeof(navgpu_global_pose) * (size_t)total;
  if (bytes > rp.up_bytes) {  // (the upload before this one has been waited for)
    uint8_t* q = nullptr;
    if ((rc = f->alloc(&q, bytes)) != NAVGPU_OK) return rc;
    f->release(rp.d_up);
    rp.d_up = q;
    rp.up_bytes = bytes;
  }
  for (uint32_t k = 0; k <= count; ++k) rp.h_off[k] = offsets[k] - offsets[0];
  if (total) {  // one upload of the poses, scattered to the robots' slots on the device
    HIP_TRY(hipMemcpyAsync(rp.d_off, rp.h_off, sizeof(uint32_t) * (count + 1), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(rp.d_up, poses_xyyaw + 3 * (size_t)offsets[0], bytes, hipMemcpyHostToDevice, f->stream));
    launch_plan_scatter(reinterpret_cast<const navgpu_global_pose*>(rp.d_up), rp.d_off, count, rp.d_poses + (size_t)first * rp.cap, rp.cap, f->stream);
    HIP_TRY(waitStream(f->stream));  // the caller's buffer and the staging area are free again
    if ((rc = checkLaunch()) != NAVGPU_OK) return rc;
  }
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t len = offsets[k + 1] - offsets[k];
    becomeResident(f, first + k, len, T ? T + 3 * (size_t)k : nullptr);
    if (len) {  // getGoalPose's input is at hand
      Robot& R = rp.robots[first + k];
      const double* g = poses_xyyaw + 3 * ((size_t)offsets[k + 1] - 1);
      toGlobal(R, navgpu_global_pose{g[0], g[1], g[2]}, R.goal);
      R.goal_known = true;
    }
  }
  return navgpu_planner_set_plan(f, first, count);  // DWAPlanner::setPlan: resetOscillationFlags
}

int navgpu_local_planner_adopt_plans(navgpu_fleet* f, uint32_t fleet_first, navgpu_navfn* h, uint32_t nav_first, uint32_t count, int32_t family,
                                     const double* T, int32_t* adopted_out) {
  if (!f || !h || !f->rangeOk(fleet_first, count) || !navfnRange(h, nav_first, count)) return NAVGPU_ERR_INVALID;
  if (family != NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER && family != NAVGPU_PLAN_FAMILY_NAVFN_ROS) return NAVGPU_ERR_INVALID;
  if (f->desc.device != h->device) return NAVGPU_ERR_INVALID;
  NavfnGuard nav_guard_(h);  // (the order of navgpu_navfn_set_costmap_from_fleet)
  FleetGuard guard_(f);
  navgpu_fleet::ResidentPlans& rp = f->rp;
  if (!rp.cap || !f->lp_configured || !f->planner_configured) return NAVGPU_ERR_STATE;
  const uint8_t maker = family == NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER ? kMadeByGlobalPlanner : kMadeByNavfnRos;
  MadePlans& m = h->made;
  for (uint32_t k = 0; k < count; ++k)
    if (m.valid.empty() || m.valid[nav_first + k] != maker) {
      g_last_error = maker == kMadeByGlobalPlanner
                         ? "navgpu_local_planner_adopt_plans: no navgpu_global_planner_make_plan since the plan's costs were set or it was planned otherwise"
                         : "navgpu_local_planner_adopt_plans: no navgpu_navfn_ros_make_plan / _plan_from_potential since the plan's costs were set or it was "
                           "planned otherwise";
      return NAVGPU_ERR_STATE;
    }
  int rc = waitAdoption(f);
  if (rc) return rc;
  std::vector<uint8_t> adopt(count, 0);
  bool any = false, too_long = false;
  for (uint32_t k = 0; k < count; ++k) {
    const int32_t np = m.rec[nav_first + k].n_poses;
    if (np > 0 && (uint32_t)np > rp.cap) too_long = true;
    adopt[k] = np > 0 && (uint32_t)np <= rp.cap;
    any = any || adopt[k];
    rp.h_off[k] = (fleet_first + k) * rp.cap;  // plan k's poses start at its robot's slot
    if (adopted_out) adopted_out[k] = adopt[k];
  }
  if (any) {
    // the NavFn stream writes the slots once the fleet's stream has finished with them, and the fleet's stream goes on once they
    // are written: two events, no device-wide wait
    HIP_TRY(hipEventRecord(rp.ev_fleet, f->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, rp.ev_fleet, 0));
    HIP_TRY(hipMemcpyAsync(rp.d_off, rp.h_off, sizeof(uint32_t) * count, hipMemcpyHostToDevice, h->stream));
    const uint32_t capacity = f->desc.n_instances * rp.cap;
    for (uint32_t k = 0; k < count;) {
      if (!adopt[k]) {
        ++k;
        continue;
      }
      uint32_t e = k;
      while (e < count && adopt[e]) ++e;
      launch_gp_plan_emit(h->nv, nav_first + k, e - k, m.d_rec + nav_first + k, rp.d_off + k, rp.d_poses, capacity, h->stream);
      k = e;
    }
    if ((rc = checkLaunch()) != NAVGPU_OK) return rc;
    HIP_TRY(hipEventRecord(rp.ev_nav, h->stream));
    rp.ev_nav_set = true;
    HIP_TRY(hipStreamWaitEvent(f->stream, rp.ev_nav, 0));
    for (uint32_t k = 0; k < count;) {
      if (!adopt[k]) {
        ++k;
        continue;
      }
      uint32_t e = k;
      while (e < count && adopt[e]) {
        becomeResident(f, fleet_first + e, (uint32_t)m.rec[nav_first + e].n_poses, T ? T + 3 * (size_t)e : nullptr);
        ++e;
      }
      if ((rc = navgpu_planner_set_plan(f, fleet_first + k, e - k)) != NAVGPU_OK) return rc;
      k = e;
    }
  }
  if (too_long) {
    g_last_error = "navgpu_local_planner_adopt_plans: a plan is longer than max_global_plan and was not adopted";
    return NAVGPU_ERR_CAPACITY;
  }
  return NAVGPU_OK;
}

int navgpu_local_planner_local_plan(navgpu_fleet* f, uint32_t instance, double* xyyaw, uint32_t capacity) {
  if (!f || instance >= f->desc.n_instances || !f->lp_configured) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->rp.residentAt(instance)) {
    const std::vector<double>& pl = f->lp[instance].local;
    const uint32_t n = (uint32_t)(pl.size() / 3);
    if (xyyaw) {
      if (capacity < n) return NAVGPU_ERR_CAPACITY;
      memcpy(xyyaw, pl.data(), sizeof(double) * pl.size());
    }
    return (int)n;
  }
  const Robot& R = f->rp.robots[instance];
  if (xyyaw) {
    if (capacity < R.loc_n) return NAVGPU_ERR_CAPACITY;
    const int rc = readSlot(f, instance, R.loc_first, R.loc_n, xyyaw);
    if (rc) return rc;
    for (uint32_t q = 0; q < R.loc_n; ++q) toGlobal(R, navgpu_global_pose{xyyaw[3 * q], xyyaw[3 * q + 1], xyyaw[3 * q + 2]}, xyyaw + 3 * q);
  }
  return (int)R.loc_n;
}

int navgpu_local_planner_windows(navgpu_fleet* f, uint32_t first, uint32_t count, navgpu_local_window* out) {
  if (!f || !out || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (!f->lp_configured) return NAVGPU_ERR_STATE;
  for (uint32_t k = 0; k < count; ++k) out[k] = f->lp[first + k].window;
  return NAVGPU_OK;
}

}  // extern "C"
