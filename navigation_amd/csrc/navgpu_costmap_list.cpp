// C-ABI host side of the costmap update for a robot list (include/navgpu.h: navgpu_costmap_stage_list, navgpu_costmap_update_list,
// navgpu_costmap_bounds_list; navgpu_obsbuf_stage_list is with the observation buffer, navgpu_obs_buffer.cpp).  The range calls
// (navgpu_host.cpp) take [first, first + count); these take instances[0 .. n_robots), strictly increasing, and launch every kernel
// once with the list in device memory where the range form passes `first`.  What both forms check and the arithmetic of the pinned
// mirrors are one copy (checkStageObservations, stageObservationMirrors, stagePoseMirrors: navgpu_host.cpp).
#include "navgpu_fleet.h"

namespace navgpu {

// the buffers of the listed calls, all or none
int reserveCostmapList(navgpu_fleet* f) {
  navgpu_fleet::CostmapList& cl = f->cml;
  if (cl.list.d) return NAVGPU_OK;
  const uint32_t n = f->desc.n_instances;
  const size_t stage_bytes = (size_t)n * (sizeof(CmStageRec) + sizeof(double) * 2 * kMaxFootprint + sizeof(ObsCsr) * f->cm.max_obs +
                                          sizeof(float) * 3 * (size_t)f->cm.max_points);
  navgpu_fleet::CostmapList nl;
  int rc = f->alloc(&nl.list.d, n);
  if (!rc) rc = f->alloc(&nl.d_stage, stage_bytes);
  if (!rc) rc = f->allocPinned(&nl.list.h, n);
  if (!rc) rc = f->allocPinned(&nl.h_stage, stage_bytes);
  if (!rc && hipEventCreateWithFlags(&nl.list.ev, hipEventDisableTiming) != hipSuccess) rc = NAVGPU_ERR_HIP;
  if (!rc && hipEventCreateWithFlags(&nl.ev_stage, hipEventDisableTiming) != hipSuccess) rc = NAVGPU_ERR_HIP;
  if (rc) {
    f->release(nl.list.d);
    f->release(nl.d_stage);
    f->releasePinned(nl.list.h);
    f->releasePinned(nl.h_stage);
    if (nl.list.ev) (void)hipEventDestroy(nl.list.ev);
    if (nl.ev_stage) (void)hipEventDestroy(nl.ev_stage);
    return rc;
  }
  cl = nl;
  return NAVGPU_OK;
}

// Precondition: the caller holds the fleet, has reserved the buffers, has waited for the mirrors and has written them for the
// listed robots.  Nothing here fails short of a HIP error.
int sendCostmapStageList(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances, bool with_points) {
  CostmapDev& cm = f->cm;
  navgpu_fleet::CostmapList& cl = f->cml;
  const bool rolling = f->desc.rolling_window != 0;
  if (cl.ev_stage_set) HIP_TRY(hipEventSynchronize(cl.ev_stage));  // the pinned block may still feed the listed stage before
  uint32_t n_fp = 0, n_obs = 0, n_pts = 0;
  for (uint32_t k = 0; k < n_robots; ++k) {
    const uint32_t i = instances[k];
    n_fp += f->hp_fpn[i];
    n_obs += f->hp_cnt[i];
    if (with_points) n_pts += f->hp_used[i];
  }
  // (<= n_instances x the per-robot capacities: the block holds them)
  const size_t o_fp = sizeof(CmStageRec) * n_robots, o_obs = o_fp + sizeof(double) * 2 * n_fp, o_pts = o_obs + sizeof(ObsCsr) * n_obs,
               bytes = o_pts + sizeof(float) * 3 * (size_t)n_pts;
  CmStageRec* rec = reinterpret_cast<CmStageRec*>(cl.h_stage);
  double* fp = reinterpret_cast<double*>(cl.h_stage + o_fp);
  ObsCsr* obs = reinterpret_cast<ObsCsr*>(cl.h_stage + o_obs);
  float* pts = reinterpret_cast<float*>(cl.h_stage + o_pts);
  uint32_t at_fp = 0, at_obs = 0, at_pts = 0;
  for (uint32_t k = 0; k < n_robots; ++k) {
    const uint32_t i = instances[k];
    CmStageRec& r = rec[k];
    memset(&r, 0, sizeof(r));
    for (int c = 0; c < 3; ++c) r.pose[c] = f->hp_pose[3 * i + c];
    if (rolling) {
      r.origin[0] = f->h_origin[2 * (size_t)i];
      r.origin[1] = f->h_origin[2 * (size_t)i + 1];
      r.shift[0] = f->hp_shift[2 * i];
      r.shift[1] = f->hp_shift[2 * i + 1];
      f->touchInputs(i, 1);  // the origins move now
    }
    r.inst = i;
    r.fp_n = f->hp_fpn[i];
    r.fp_off = at_fp;
    r.obs_count = f->hp_cnt[i];
    r.obs_off = at_obs;
    r.n_points = with_points ? f->hp_used[i] : 0;
    r.pts_off = at_pts;
    memcpy(fp + 2 * (size_t)at_fp, f->hp_fpw + (size_t)i * kMaxFootprint * 2, sizeof(double) * 2 * r.fp_n);
    memcpy(obs + at_obs, f->hp_obs + (size_t)i * cm.max_obs, sizeof(ObsCsr) * r.obs_count);
    if (r.n_points) memcpy(pts + 3 * (size_t)at_pts, f->hp_pts + (size_t)i * cm.max_points * 3, sizeof(float) * 3 * r.n_points);
    at_fp += r.fp_n;
    at_obs += r.obs_count;
    at_pts += r.n_points;
  }
  HIP_TRY(hipMemcpyAsync(cl.d_stage, cl.h_stage, bytes, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipEventRecord(cl.ev_stage, f->stream));
  cl.ev_stage_set = true;
  launch_cm_stage_scatter(cm, reinterpret_cast<const CmStageRec*>(cl.d_stage), reinterpret_cast<const double*>(cl.d_stage + o_fp),
                          reinterpret_cast<const ObsCsr*>(cl.d_stage + o_obs), reinterpret_cast<const float*>(cl.d_stage + o_pts), rolling ? 1 : 0,
                          n_robots, f->stream);
  if (f->cycles_in_flight > 1) {  // behind the copy, as the range stage records it
    HIP_TRY(hipEventRecord(f->ev_cm_h2d, f->stream));
    f->ev_cm_set = true;
  }
  if (rolling) {
    f->shift_pending = true;
    f->shift_listed = true;
    f->shift_list.assign(instances, instances + n_robots);
  }
  return checkLaunch();
}

}  // namespace navgpu

extern "C" {

int navgpu_costmap_stage_list(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances, const double* poses, const navgpu_observation* obs,
                              uint32_t n_obs, const float* points, uint32_t n_points_total) {
  if (!f || !poses || !listOk(f, n_robots, instances) || (n_obs && (!obs || (!points && n_points_total)))) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  if (f->desc.rolling_window && f->shift_pending) return NAVGPU_ERR_STATE;  // previous stage not consumed by an update yet
  const RobotSet set{0, n_robots, instances};
  int rc = checkStageObservations(f, set, obs, n_obs, n_points_total);
  if (rc == NAVGPU_OK) rc = reserveCostmapList(f);
  if (rc != NAVGPU_OK) return rc;
  HIP_TRY(f->waitMirrors(f->ev_cm_h2d, f->ev_cm_set));  // the pinned mirrors may still feed an earlier copy, and so may the packed block
  stageObservationMirrors(f, set, obs, n_obs, points);
  stagePoseMirrors(f, set, poses);
  return sendCostmapStageList(f, n_robots, instances, true);
}

// rolling window: navgpu_costmap_update's applyPendingShift for the robots of the list.  The ping-pong swap is fleet-wide, so the
// listed robots' grids are shifted into the targets (k_shift, the fills of the range form) and copied back (k_shift_back): the
// fleet's pointers, cm.master / pl.master among them, stay where they were, and so does every byte of the other robots.
// (the caller has checked that the list is the one staged)
static void applyPendingShiftList(navgpu_fleet* f, uint32_t n_robots, RobotList robots) {
  CostmapDev& cm = f->cm;
  if (!(f->desc.rolling_window && f->shift_pending)) return;
  launch_shift_u8(cm.master, cm.master_alt, cm, robots, n_robots, cm.master_default, f->stream);
  launch_shift_back_u8(cm.master_alt, cm.master, cm, robots, n_robots, f->stream);
  if (cm.obst) {
    launch_shift_u8(cm.obst, cm.obst_alt, cm, robots, n_robots, cm.obstacle_default, f->stream);
    launch_shift_back_u8(cm.obst_alt, cm.obst, cm, robots, n_robots, f->stream);
  }
  if (cm.voxel) {
    launch_shift_u32(cm.voxel, cm.voxel_alt, cm, robots, n_robots, 0x0000FFFFu, f->stream);
    launch_shift_back_u32(cm.voxel_alt, cm.voxel, cm, robots, n_robots, f->stream);
  }
  f->shift_pending = false;
  f->shift_listed = false;
}

// LayeredCostmap::updateMap (layered_costmap.cpp:82-150) of the listed robots: the launches of navgpu_costmap_update, each once
int navgpu_costmap_update_list(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances) {
  if (!f || !listOk(f, n_robots, instances)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  CostmapDev& cm = f->cm;
  if ((cm.layers & NAVGPU_LAYER_INFLATION) && !f->inflation_configured) return NAVGPU_ERR_STATE;
  // the set staged last is the set the update names, and a range stage is updated by the range call
  if (f->desc.rolling_window && f->shift_pending &&
      (!f->shift_listed || f->shift_list.size() != n_robots || !std::equal(instances, instances + n_robots, f->shift_list.begin())))
    return NAVGPU_ERR_STATE;
  int rc = reserveCostmapList(f);
  if (rc != NAVGPU_OK) return rc;
  if ((rc = f->cml.list.send(f, instances, n_robots)) != NAVGPU_OK) return rc;
  const RobotList robots{f->cml.list.d};
  for (uint32_t k = 0; k < n_robots; ++k) f->touchInputs(instances[k], 1);
  applyPendingShiftList(f, n_robots, robots);
  PROFILED(f, NAVGPU_K_OBSTACLE, launch_obstacle(cm, robots, n_robots, nullptr, 0, f->stream));
  for (uint32_t k = 0; k < n_robots; ++k) f->obs_consumed[instances[k]] = 1;
  PROFILED(f, NAVGPU_K_MERGE, launch_merge(cm, robots, n_robots, nullptr, f->stream));
  if (cm.layers & NAVGPU_LAYER_INFLATION) PROFILED(f, NAVGPU_K_INFLATE, launch_inflate(cm, robots, n_robots, nullptr, f->stream));
  return checkLaunch();
}

// the cell boxes of the listed robots' last updateMap (layered_costmap.cpp:113-135), boxes[k] for instances[k]
int navgpu_costmap_bounds_list(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances, int32_t* boxes) {
  if (!f || !boxes || !listOk(f, n_robots, instances)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  const uint32_t lo = instances[0], span = instances[n_robots - 1] - lo + 1;  // one copy: the states between the first and the last
  std::vector<InstCostmapState> st(span);
  HIP_TRY(hipMemcpyAsync(st.data(), f->cm.state + lo, sizeof(InstCostmapState) * span, hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  for (uint32_t k = 0; k < n_robots; ++k)
    for (int c = 0; c < 4; ++c) boxes[4 * k + c] = st[instances[k] - lo].box[c];
  return NAVGPU_OK;
}

}  // extern "C"
