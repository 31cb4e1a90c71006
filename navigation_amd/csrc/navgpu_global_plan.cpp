// navgpu_global_planner_make_plan / _plans / _potential_grid: GlobalPlanner::makePlan end to end for a batch of plans - host side
// (global_plan_kernels.hip has the kernels, navgpu_navfn.cpp the handle and the expansion's entry points; include/navgpu.h the contract).
#include "navgpu_navfn.h"

using navgpu::costmapWorldToMap;

// navgpu_global_planner_plans and navgpu_navfn_ros_plans: the plans of the range as their maker's records describe them
int assembleMadePlans(navgpu_navfn* h, uint32_t first, uint32_t count, uint8_t maker, uint32_t capacity, navgpu_global_pose* poses, uint32_t* offsets) {
  if (!h || !offsets || (!poses && capacity) || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  NavfnGuard guard_(h);
  MadePlans& m = h->made;
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; ++k) {
    if (m.valid.empty() || m.valid[first + k] != maker) {
      g_last_error = maker == kMadeByGlobalPlanner
                         ? "navgpu_global_planner_plans: no navgpu_global_planner_make_plan since the plan's costs were set or it was planned otherwise"
                         : "navgpu_navfn_ros_plans: no navgpu_navfn_ros_make_plan / _plan_from_potential since the plan's costs were set or it was planned otherwise";
      return NAVGPU_ERR_STATE;
    }
    total += (uint64_t)m.rec[first + k].n_poses;
  }
  // one buffer, one copy: the offsets (padded to the poses' alignment), then the poses that fit
  const size_t n_write = (size_t)std::min<uint64_t>(total, capacity);
  const size_t off_bytes = ((size_t)(count + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
  const size_t bytes = off_bytes + n_write * sizeof(navgpu_global_pose);
  int rc = growBuffer(h, &m.d_out, &m.out_bytes, bytes);
  if (rc) return rc;
  uint32_t* d_offsets = reinterpret_cast<uint32_t*>(m.d_out);
  navgpu_global_pose* d_poses = reinterpret_cast<navgpu_global_pose*>(m.d_out + off_bytes);
  launch_gp_plan_scan(m.d_rec + first, count, d_offsets, h->stream);
  launch_gp_plan_emit(h->nv, first, count, m.d_rec + first, d_offsets, d_poses, (uint32_t)n_write, h->stream);
  m.h_out.resize(bytes);
  HIP_TRY(hipMemcpyAsync(m.h_out.data(), m.d_out, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;
  memcpy(offsets, m.h_out.data(), sizeof(uint32_t) * (count + 1));
  if (n_write) memcpy(poses, m.h_out.data() + off_bytes, n_write * sizeof(navgpu_global_pose));
  return NAVGPU_OK;
}

extern "C" {

int navgpu_global_planner_make_plan(navgpu_navfn* h, uint32_t first, uint32_t count, const navgpu_global_planner_params* gp,
                                    const navgpu_make_plan_options* opt, const double* frames, const double* starts, const double* goals,
                                    navgpu_make_plan_result* results) {
  if (!h || !gp || !opt || !frames || !starts || !goals || !results || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (gp->lethal_cost < 2 || gp->lethal_cost > 255 || gp->neutral_cost < 0 || gp->neutral_cost > 255) return NAVGPU_ERR_INVALID;
  if (opt->orientation_mode < NAVGPU_ORIENT_NONE || opt->orientation_mode > NAVGPU_ORIENT_FORWARD_THEN_INTERPOLATE) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < count; ++k)
    if (!(frames[3 * k + 2] > 0.0) || !std::isfinite(frames[3 * k + 2])) {
      g_last_error = "navgpu_global_planner_make_plan: resolution must be positive";
      return NAVGPU_ERR_INVALID;
    }
  if (opt->wavefront && !gp->use_dijkstra) {
    g_last_error = "navgpu_global_planner_make_plan: the wavefront expansion is Dijkstra only";
    return NAVGPU_ERR_INVALID;
  }
  NavfnGuard guard_(h);
  NavfnDev& nv = h->nv;
  int rc = reserveMadePlans(h);
  if (rc) return rc;
  MadePlans& m = h->made;
  m.forget(first, count);

  // makePlan up to clearRobotCell (planner_core.cpp:250-286): cells, map coordinates, statuses
  const double convert_offset = gp->old_navfn_behavior ? 0.0 : 0.5;
  std::vector<double> xy_start((size_t)count * 2, 0.0), xy_goal((size_t)count * 2, 0.0);
  std::vector<int32_t> goal_cells((size_t)count * 2, 0), clear_cells(count, -1);
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_make_plan_result& r = results[k];
    r = navgpu_make_plan_result{};
    const double ox = frames[3 * k], oy = frames[3 * k + 1], res = frames[3 * k + 2];
    const double *s = starts + 3 * k, *g = goals + 3 * k;
    if (!costmapWorldToMap(s[0], s[1], ox, oy, res, nv.nx, nv.ny, r.start_cell)) {
      r.start_cell[0] = r.start_cell[1] = 0;
      r.status = NAVGPU_MAKE_PLAN_START_OFF_MAP;
      continue;
    }
    if (!costmapWorldToMap(g[0], g[1], ox, oy, res, nv.nx, nv.ny, r.goal_cell)) {
      r.goal_cell[0] = r.goal_cell[1] = 0;
      r.status = NAVGPU_MAKE_PLAN_GOAL_OFF_MAP;
      continue;
    }
    double sx = r.start_cell[0], sy = r.start_cell[1], gx = r.goal_cell[0], gy = r.goal_cell[1];
    if (!gp->old_navfn_behavior) {  // GlobalPlanner::worldToMap (:201-215), its return value ignored as makePlan ignores it
      sx = (s[0] - ox) / res - convert_offset;
      sy = (s[1] - oy) / res - convert_offset;
      gx = (g[0] - ox) / res - convert_offset;
      gy = (g[1] - oy) / res - convert_offset;
    }
    if (!(sx >= 2 && sy >= 2 && sx < nv.nx - 3 && sy < nv.ny - 3 && gx >= 1 && gy >= 1 && gx < nv.nx - 1 && gy < nv.ny - 1)) {
      r.status = NAVGPU_MAKE_PLAN_BORDER;  // (navgpu_global_planner_plan's limit: the reference reads outside its arrays there)
      continue;
    }
    xy_start[2 * k] = sx, xy_start[2 * k + 1] = sy;
    xy_goal[2 * k] = gx, xy_goal[2 * k + 1] = gy;
    goal_cells[2 * k] = r.goal_cell[0], goal_cells[2 * k + 1] = r.goal_cell[1];
    clear_cells[k] = r.start_cell[0] + nv.nx * r.start_cell[1];
  }
  double* d_starts = h->d_xy;
  double* d_goals = h->d_xy + (size_t)2 * h->n;
  HIP_TRY(hipMemcpyAsync(d_starts, xy_start.data(), sizeof(double) * 2 * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_goals, xy_goal.data(), sizeof(double) * 2 * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_goal, goal_cells.data(), sizeof(int32_t) * 2 * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(m.d_clear, clear_cells.data(), sizeof(int32_t) * count, hipMemcpyHostToDevice, h->stream));
  launch_gp_clear_cells(nv, first, count, m.d_clear, h->stream);  // clearRobotCell

  if (!opt->wavefront && !gp->use_dijkstra && !h->d_heap) {
    uint64_t* q = nullptr;  // (as navgpu_global_planner_plan)
    rc = h->alloc(&q, (size_t)h->n * nv.ns_padded);
    if (rc) return rc;
    h->d_heap = q;
  }
  // the existing launchers, once per maximal run [a, b) of plans to attempt: they take plan first + a + i from element i of their arrays
  for (uint32_t a = 0; a < count;) {
    if (clear_cells[a] < 0) {
      ++a;
      continue;
    }
    uint32_t b = a;
    while (b < count && clear_cells[b] >= 0) ++b;
    const uint32_t run = b - a;
    if (!opt->wavefront) {
      launch_gp_plan(nv, first + a, run, *gp, d_starts + 2 * a, d_goals + 2 * a, h->d_goal + 2 * a, h->d_heap, h->stream);
      std::fill(h->final_array.begin() + first + a, h->final_array.begin() + first + b, (uint8_t)0);
    } else {
      std::vector<int32_t> seed_cells, stop;
      std::vector<float> seed_vals;
      gpWavefrontSeeds(nv.nx, *gp, run, &xy_start[2 * a], &xy_goal[2 * a], seed_cells, seed_vals, stop);
      const NavfnWfRule rule = gpWavefrontRule(*gp);
      rc = runWavefront(h, first + a, run, rule, seed_cells.data(), seed_vals.data(), stop.data(), 1);
      if (rc) return rc;
      launch_gp_wf_finish(nv, first + a, run, *gp, d_starts + 2 * a, d_goals + 2 * a, h->d_goal + 2 * a, h->stream);
    }
    a = b;
  }
  HIP_TRY(hipMemcpyAsync(h->h_results + first, nv.results + first, sizeof(navgpu_navfn_result) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;

  for (uint32_t k = 0; k < count; ++k) {
    navgpu_make_plan_result& r = results[k];
    navgpu_navfn_result& nr = h->h_results[first + k];
    if (clear_cells[k] < 0) nr = navgpu_navfn_result{};  // not attempted: navgpu_navfn_path must not hand out an earlier call's
    r.found = nr.found;
    r.cycles = nr.cycles;
    r.start_potential = nr.start_potential;
    if (clear_cells[k] >= 0 && !(nr.found && nr.path_length > 0)) r.status = NAVGPU_MAKE_PLAN_NO_PLAN;
    navgpu::GpPlanRec& rec = m.rec[first + k];
    rec = navgpu::GpPlanRec{};
    if (r.status == NAVGPU_MAKE_PLAN_OK) {
      r.n_poses = nr.path_length + (gp->old_navfn_behavior ? 2 : 1);
      rec.origin_x = frames[3 * k], rec.origin_y = frames[3 * k + 1], rec.resolution = frames[3 * k + 2];
      rec.convert_offset = convert_offset;
      rec.start_yaw = starts[3 * k + 2];
      rec.goal_x = goals[3 * k], rec.goal_y = goals[3 * k + 1], rec.goal_yaw = goals[3 * k + 2];
      rec.n_path = nr.path_length;
      rec.n_poses = r.n_poses;
      rec.mode = opt->orientation_mode;
    }
    m.valid[first + k] = kMadeByGlobalPlanner;
  }
  HIP_TRY(hipMemcpyAsync(m.d_rec + first, m.rec.data() + first, sizeof(navgpu::GpPlanRec) * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_global_planner_plans(navgpu_navfn* h, uint32_t first, uint32_t count, uint32_t capacity, navgpu_global_pose* poses, uint32_t* offsets) {
  return assembleMadePlans(h, first, count, kMadeByGlobalPlanner, capacity, poses, offsets);
}

int navgpu_global_planner_potential_grid(navgpu_navfn* h, uint32_t first, uint32_t count, int32_t publish_scale, int8_t* grids, float* maxima) {
  if (!h || !grids || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  NavfnGuard guard_(h);
  const NavfnDev& nv = h->nv;
  int rc = reserveMadePlans(h);
  if (rc) return rc;
  MadePlans& m = h->made;
  const size_t bytes = (size_t)count * nv.ns;
  rc = growBuffer(h, &m.d_grids, &m.grid_bytes, bytes);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(m.d_alt, h->final_array.data() + first, count, hipMemcpyHostToDevice, h->stream));
  launch_gp_potential_grid(nv, first, count, m.d_alt, publish_scale, m.d_grids, m.d_maxima, h->stream);
  HIP_TRY(hipMemcpyAsync(grids, m.d_grids, bytes, hipMemcpyDeviceToHost, h->stream));
  if (maxima) HIP_TRY(hipMemcpyAsync(maxima, m.d_maxima, sizeof(float) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  return checkLaunch();
}

}  // extern "C"
