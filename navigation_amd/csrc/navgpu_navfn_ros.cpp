// navgpu_navfn_ros_*: navfn::NavfnROS (navfn/src/navfn_ros.cpp) round the NavFn batch - host side
// (navfn_ros_kernels.hip has the kernels, navgpu_navfn.cpp the handle and the expansion's entry points; include/navgpu.h the contract).
#include "navgpu_navfn.h"

using navgpu::costmapWorldToMap;
using navgpu::kNrMaxWindow;
using navgpu::NrBest;
using navgpu::NrCloudPlan;
using navgpu::NrCloudPoint;
using navgpu::NrPathJob;
using navgpu::NrWindow;

namespace {

// `p = centre - tolerance; while (p <= centre + tolerance) { ...; p += resolution; }` (navfn_ros.cpp:308-326, 140-151): the values
// p takes, appended to seq.  -> how many, or -1 beyond the library's limit (a sum that stops moving never ends in the reference)
int windowSequence(double centre, double tolerance, double resolution, std::vector<double>& seq) {
  int n = 0;
  for (double p = centre - tolerance; p <= centre + tolerance; p += resolution) {
    if (++n > kNrMaxWindow) return -1;
    seq.push_back(p);
  }
  return n;
}

bool framesOk(const char* call, const double* frames, uint32_t count) {
  for (uint32_t k = 0; k < count; ++k)
    if (!(frames[3 * k + 2] > 0.0) || !std::isfinite(frames[3 * k + 2])) {
      g_last_error = std::string(call) + ": resolution must be positive";
      return false;
    }
  return true;
}

int reserveRos(navgpu_navfn* h) {
  NavfnRosState& r = h->ros;
  if (r.d_cloud_plans) return NAVGPU_OK;
  r.nav_start.assign(h->n, 0);
  r.nav_goal.assign((size_t)h->n * 2, 0);
  int rc = reserveMadePlans(h);
  if (!rc && !r.d_path) rc = h->alloc(&r.d_path, h->n);
  if (!rc) rc = h->alloc(&r.d_cloud_plans, h->n);  // last: its presence says the others exist
  return rc;
}

// the window jobs of a call and their sequences, uploaded; best[] is sized for them
int uploadWindows(navgpu_navfn* h, const std::vector<NrWindow>& win, const std::vector<double>& seq) {
  NavfnRosState& r = h->ros;
  int rc = growBuffer(h, &r.d_win, &r.win_cap, win.size());
  if (!rc) rc = growBuffer(h, &r.d_best, &r.best_cap, win.size());
  if (!rc) rc = growBuffer(h, &r.d_seq, &r.seq_cap, std::max<size_t>(seq.size(), 1));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(r.d_win, win.data(), sizeof(NrWindow) * win.size(), hipMemcpyHostToDevice, h->stream));
  if (!seq.empty()) HIP_TRY(hipMemcpyAsync(r.d_seq, seq.data(), sizeof(double) * seq.size(), hipMemcpyHostToDevice, h->stream));
  return NAVGPU_OK;
}

// NavFn::setGoal / setStart + calcNavFnDijkstra(at_start) of the plans first + [a, b), whose cells are elements a .. b - 1 of the
// handle's d_goal / d_start: the bit-exact launcher, or the tiled wavefront as navgpu_navfn_plan_wavefront runs it
int expandRun(navgpu_navfn* h, uint32_t first, uint32_t a, uint32_t b, const int32_t* goals, const int32_t* starts, int wavefront, int at_start) {
  NavfnDev& nv = h->nv;
  const uint32_t run = b - a;
  if (!wavefront) {
    launch_navfn_plan(nv, first + a, run, h->d_goal + 2 * a, h->d_start + 2 * a, 0, at_start, h->stream);
    std::fill(h->final_array.begin() + first + a, h->final_array.begin() + first + b, (uint8_t)0);
    return NAVGPU_OK;
  }
  std::vector<int32_t> seed_cells((size_t)run * 4, -1), stop(run);
  std::vector<float> seed_vals((size_t)run * 4, 0.0f);
  for (uint32_t q = 0; q < run; ++q) {
    seed_cells[4 * q] = goals[2 * (a + q)] + goals[2 * (a + q) + 1] * nv.nx;  // initCost(goal, 0)
    stop[q] = starts[2 * (a + q)] + starts[2 * (a + q) + 1] * nv.nx;
  }
  navgpu::NavfnWfRule rule{};
  rule.quadratic = 1;
  rule.outline = 1;
  const int rc = runWavefront(h, first + a, run, rule, seed_cells.data(), seed_vals.data(), stop.data(), at_start);
  if (rc) return rc;
  launch_navfn_wf_path(nv, first + a, run, h->d_goal + 2 * a, h->d_start + 2 * a, h->stream);
  return NAVGPU_OK;
}

// every maximal run of plans with attempt[k] set goes through expandRun
int expandAttempted(navgpu_navfn* h, uint32_t first, uint32_t count, const std::vector<uint8_t>& attempt, const std::vector<int32_t>& goals,
                    const std::vector<int32_t>& starts, int wavefront, int at_start) {
  HIP_TRY(hipMemcpyAsync(h->d_goal, goals.data(), sizeof(int32_t) * 2 * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_start, starts.data(), sizeof(int32_t) * 2 * count, hipMemcpyHostToDevice, h->stream));
  for (uint32_t a = 0; a < count;) {
    if (!attempt[a]) {
      ++a;
      continue;
    }
    uint32_t b = a;
    while (b < count && attempt[b]) ++b;
    const int rc = expandRun(h, first, a, b, goals.data(), starts.data(), wavefront, at_start);
    if (rc) return rc;
    a = b;
  }
  return NAVGPU_OK;
}

}  // namespace

extern "C" {

int navgpu_navfn_ros_make_plan(navgpu_navfn* h, uint32_t first, uint32_t count, const navgpu_navfn_ros_params* params, const double* frames,
                               const double* starts, const double* goals, const double* tolerances, navgpu_navfn_ros_result* results) {
  if (!h || !params || !frames || !starts || !goals || !tolerances || !results || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (!framesOk("navgpu_navfn_ros_make_plan", frames, count)) return NAVGPU_ERR_INVALID;
  NavfnGuard guard_(h);
  NavfnDev& nv = h->nv;

  // makePlan up to the expansion (navfn_ros.cpp:244-296): cells and statuses; the window's sequences (:308-326)
  std::vector<uint8_t> attempt(count, 0);
  std::vector<int32_t> robot_cells((size_t)count * 2, 0), goal_cells((size_t)count * 2, 0);
  std::vector<NrWindow> win(count, NrWindow{});
  std::vector<double> seq;
  std::vector<navgpu_navfn_ros_result> out(count, navgpu_navfn_ros_result{});
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_navfn_ros_result& r = out[k];
    const double ox = frames[3 * k], oy = frames[3 * k + 1], res = frames[3 * k + 2];
    const double *s = starts + 3 * k, *g = goals + 3 * k;
    const double tolerance = tolerances[k];
    if (!costmapWorldToMap(s[0], s[1], ox, oy, res, nv.nx, nv.ny, r.start_cell)) {
      r.start_cell[0] = r.start_cell[1] = 0;
      r.status = NAVGPU_MAKE_PLAN_START_OFF_MAP;
      continue;
    }
    if (!costmapWorldToMap(g[0], g[1], ox, oy, res, nv.nx, nv.ny, r.goal_cell)) {
      r.goal_cell[0] = r.goal_cell[1] = 0;  // mx = my = 0 (:287-288)
      if (tolerance <= 0.0) {
        r.status = NAVGPU_MAKE_PLAN_GOAL_OFF_MAP;
        continue;
      }
    }
    NrWindow& w = win[k];
    w.origin_x = ox, w.origin_y = oy, w.resolution = res;
    w.goal_x = g[0], w.goal_y = g[1];
    w.w_dist = params->tolerance_weight_dist_from_goal, w.w_len = params->tolerance_weight_path_length;
    w.plan = k;
    w.seq = (uint32_t)seq.size();
    const int wy = windowSequence(g[1], tolerance, res, seq);
    const int wx = wy < 0 ? -1 : windowSequence(g[0], tolerance, res, seq);
    if (wx < 0) {
      g_last_error = "navgpu_navfn_ros_make_plan: more than 4096 window candidates per axis";
      return NAVGPU_ERR_INVALID;
    }
    w.ny = (uint32_t)wy, w.nx = (uint32_t)wx;
    attempt[k] = 1;
    robot_cells[2 * k] = r.start_cell[0], robot_cells[2 * k + 1] = r.start_cell[1];
    goal_cells[2 * k] = r.goal_cell[0], goal_cells[2 * k + 1] = r.goal_cell[1];
  }
  int rc = reserveRos(h);
  if (rc) return rc;
  MadePlans& m = h->made;
  NavfnRosState& ros = h->ros;
  m.forget(first, count);

  // planner_->setStart(map_goal); setGoal(map_start); calcNavFnDijkstra(true) (:295-299): NavFn's goal is the robot's cell
  rc = expandAttempted(h, first, count, attempt, robot_cells, goal_cells, params->wavefront, 1);
  if (rc) return rc;

  std::vector<NrPathJob> jobs(count, NrPathJob{});
  for (uint32_t k = 0; k < count; ++k) {
    win[k].use_alt = h->final_array[first + k];
    NrPathJob& j = jobs[k];
    j.start[0] = j.start[1] = -1;
    j.from_best = attempt[k];
    j.goal[0] = robot_cells[2 * k], j.goal[1] = robot_cells[2 * k + 1];
    j.use_alt = h->final_array[first + k];
  }
  rc = uploadWindows(h, win, seq);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ros.d_path, jobs.data(), sizeof(NrPathJob) * count, hipMemcpyHostToDevice, h->stream));
  launch_nr_window(nv, first, ros.d_win, ros.d_seq, count, 0, ros.d_best, h->stream);
  // getPlanFromPotential (:426-437): setStart(best cell), calcPath(nx * 4) over the same potential array.  The gradx / grady the
  // expansion's own calcPath(nx * ny / 2) memoised are a pure function of potarr, so this walk reads what it would compute
  // itself: the path is the same with the caches kept (as the reference keeps them) or zeroed.
  launch_nr_path(nv, first, count, ros.d_path, ros.d_best, h->stream);
  std::vector<NrBest> best(count);
  HIP_TRY(hipMemcpyAsync(best.data(), ros.d_best, sizeof(NrBest) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(jobs.data(), ros.d_path, sizeof(NrPathJob) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(h->h_results + first, nv.results + first, sizeof(navgpu_navfn_result) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;

  for (uint32_t k = 0; k < count; ++k) {
    navgpu_navfn_ros_result& r = out[k];
    navgpu::GpPlanRec& rec = m.rec[first + k];
    rec = navgpu::GpPlanRec{};
    if (!attempt[k]) {
      h->h_results[first + k] = navgpu_navfn_result{};  // navgpu_navfn_path must not hand out an earlier call's
    } else {
      const NrBest& b = best[k];
      r.found = jobs[k].first_pass.found;
      r.cycles = jobs[k].first_pass.cycles;
      r.start_potential = jobs[k].first_pass.start_potential;
      r.candidates = b.candidates;
      ros.nav_start[first + k] = r.goal_cell[0] + nv.nx * r.goal_cell[1];
      ros.nav_goal[2 * (first + k)] = r.start_cell[0], ros.nav_goal[2 * (first + k) + 1] = r.start_cell[1];
      r.best_cell[0] = r.best_cell[1] = -1;
      if (b.index >= 0) {
        r.best_cell[0] = b.cell[0], r.best_cell[1] = b.cell[1];
        r.best_x = b.x, r.best_y = b.y, r.best_cost = b.cost;
        ros.nav_start[first + k] = b.cell[0] + nv.nx * b.cell[1];
      }
      if (b.index >= 0 && jobs[k].length > 0) {
        r.n_poses = jobs[k].length + 1;  // the path reversed, then best_pose with the goal's orientation (:333-335)
        rec.origin_x = frames[3 * k], rec.origin_y = frames[3 * k + 1], rec.resolution = frames[3 * k + 2];
        rec.goal_x = b.x, rec.goal_y = b.y, rec.goal_yaw = goals[3 * k + 2];
        rec.n_path = jobs[k].length;
        rec.n_poses = r.n_poses;
        rec.mode = NAVGPU_ORIENT_NONE;
      } else {
        r.status = NAVGPU_MAKE_PLAN_NO_PLAN;
        // without a best cell nothing walked a second time and the path buffer still holds the expansion's own walk; after a
        // failed second walk it holds that walk's points: navgpu_navfn_path hands out neither
        h->h_results[first + k].found = 0;
        h->h_results[first + k].path_length = 0;
      }
    }
    m.valid[first + k] = kMadeByNavfnRos;
    results[k] = r;
  }
  HIP_TRY(hipMemcpyAsync(m.d_rec + first, m.rec.data() + first, sizeof(navgpu::GpPlanRec) * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_navfn_ros_plans(navgpu_navfn* h, uint32_t first, uint32_t count, uint32_t capacity, navgpu_global_pose* poses, uint32_t* offsets) {
  return assembleMadePlans(h, first, count, kMadeByNavfnRos, capacity, poses, offsets);
}

int navgpu_navfn_ros_plan_from_potential(navgpu_navfn* h, uint32_t first, uint32_t count, const double* frames, const double* goals,
                                         navgpu_navfn_ros_result* results) {
  if (!h || !frames || !goals || !results || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (!framesOk("navgpu_navfn_ros_plan_from_potential", frames, count)) return NAVGPU_ERR_INVALID;
  NavfnGuard guard_(h);
  NavfnDev& nv = h->nv;
  int rc = reserveRos(h);
  if (rc) return rc;
  MadePlans& m = h->made;
  NavfnRosState& ros = h->ros;
  m.forget(first, count);
  // NavFn's goal stays what the last navgpu_navfn_ros_make_plan / _compute_potential on the plan set
  std::vector<NrPathJob> jobs(count, NrPathJob{});
  std::vector<navgpu_navfn_ros_result> out(count, navgpu_navfn_ros_result{});
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_navfn_ros_result& r = out[k];
    NrPathJob& j = jobs[k];
    j.start[0] = j.start[1] = -1;
    j.use_alt = h->final_array[first + k];
    j.goal[0] = ros.nav_goal[2 * (first + k)], j.goal[1] = ros.nav_goal[2 * (first + k) + 1];
    r.start_cell[0] = j.goal[0], r.start_cell[1] = j.goal[1];
    r.best_cell[0] = r.best_cell[1] = -1;
    if (!costmapWorldToMap(goals[3 * k], goals[3 * k + 1], frames[3 * k], frames[3 * k + 1], frames[3 * k + 2], nv.nx, nv.ny, r.goal_cell)) {
      r.goal_cell[0] = r.goal_cell[1] = 0;
      r.status = NAVGPU_MAKE_PLAN_GOAL_OFF_MAP;
      continue;
    }
    j.start[0] = r.goal_cell[0], j.start[1] = r.goal_cell[1];
    ros.nav_start[first + k] = r.goal_cell[0] + nv.nx * r.goal_cell[1];  // planner_->setStart(map_goal) (:430)
  }
  HIP_TRY(hipMemcpyAsync(ros.d_path, jobs.data(), sizeof(NrPathJob) * count, hipMemcpyHostToDevice, h->stream));
  // calcPath(nx * 4) over the potential the plan holds (:432); the memoised gradients are a pure function of it (see make_plan)
  launch_nr_path(nv, first, count, ros.d_path, nullptr, h->stream);
  HIP_TRY(hipMemcpyAsync(jobs.data(), ros.d_path, sizeof(NrPathJob) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(h->h_results + first, nv.results + first, sizeof(navgpu_navfn_result) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_navfn_ros_result& r = out[k];
    navgpu::GpPlanRec& rec = m.rec[first + k];
    rec = navgpu::GpPlanRec{};
    if (r.status == NAVGPU_MAKE_PLAN_OK) {
      r.found = jobs[k].length > 0;
      r.cycles = jobs[k].first_pass.cycles;
      r.start_potential = h->h_results[first + k].start_potential;
      if (jobs[k].length > 0) {
        r.n_poses = jobs[k].length;  // the path reversed; no goal is appended (:440-456)
        rec.origin_x = frames[3 * k], rec.origin_y = frames[3 * k + 1], rec.resolution = frames[3 * k + 2];
        rec.n_path = rec.n_poses = r.n_poses;
        rec.mode = NAVGPU_ORIENT_NONE;
      } else {
        r.status = NAVGPU_MAKE_PLAN_NO_PLAN;
      }
    } else {
      h->h_results[first + k].found = 0;  // the path buffer still holds an earlier walk: navgpu_navfn_path must not hand it out
      h->h_results[first + k].path_length = 0;
    }
    m.valid[first + k] = kMadeByNavfnRos;
    results[k] = r;
  }
  HIP_TRY(hipMemcpyAsync(m.d_rec + first, m.rec.data() + first, sizeof(navgpu::GpPlanRec) * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(waitStream(h->stream));
  return NAVGPU_OK;
}

int navgpu_navfn_ros_compute_potential(navgpu_navfn* h, uint32_t first, uint32_t count, const navgpu_navfn_ros_params* params, const double* frames,
                                       const double* points, navgpu_navfn_ros_result* results) {
  if (!h || !params || !frames || !points || !results || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (!framesOk("navgpu_navfn_ros_compute_potential", frames, count)) return NAVGPU_ERR_INVALID;
  NavfnGuard guard_(h);
  NavfnDev& nv = h->nv;
  int rc = reserveRos(h);
  if (rc) return rc;
  NavfnRosState& ros = h->ros;
  h->made.forget(first, count);
  std::vector<uint8_t> attempt(count, 0);
  std::vector<int32_t> goal_cells((size_t)count * 2, 0), start_cells((size_t)count * 2, 0);  // map_start = (0, 0) (:185-187)
  std::vector<navgpu_navfn_ros_result> out(count, navgpu_navfn_ros_result{});
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_navfn_ros_result& r = out[k];
    r.best_cell[0] = r.best_cell[1] = -1;
    if (!costmapWorldToMap(points[2 * k], points[2 * k + 1], frames[3 * k], frames[3 * k + 1], frames[3 * k + 2], nv.nx, nv.ny, r.goal_cell)) {
      r.goal_cell[0] = r.goal_cell[1] = 0;
      r.status = NAVGPU_MAKE_PLAN_GOAL_OFF_MAP;
      continue;
    }
    attempt[k] = 1;
    goal_cells[2 * k] = r.goal_cell[0], goal_cells[2 * k + 1] = r.goal_cell[1];
  }
  rc = expandAttempted(h, first, count, attempt, goal_cells, start_cells, params->wavefront, 0);  // calcNavFnDijkstra() (:196)
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h->h_results + first, nv.results + first, sizeof(navgpu_navfn_result) * count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;
  for (uint32_t k = 0; k < count; ++k) {
    navgpu_navfn_ros_result& r = out[k];
    navgpu_navfn_result& nr = h->h_results[first + k];
    if (!attempt[k]) {
      nr = navgpu_navfn_result{};
    } else {
      r.found = nr.found;
      r.cycles = nr.cycles;
      r.start_potential = nr.start_potential;
      ros.nav_start[first + k] = 0;
      ros.nav_goal[2 * (first + k)] = r.goal_cell[0], ros.nav_goal[2 * (first + k) + 1] = r.goal_cell[1];
    }
    results[k] = r;
  }
  return NAVGPU_OK;
}

int navgpu_navfn_ros_point_potential(navgpu_navfn* h, uint32_t first, uint32_t count, const double* frames, const uint32_t* query_counts,
                                     const double* points, double* potentials) {
  if (!h || !frames || !query_counts || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (!framesOk("navgpu_navfn_ros_point_potential", frames, count)) return NAVGPU_ERR_INVALID;
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; ++k) total += query_counts[k];
  if (total > 0x7FFFFFFFu || (total && (!points || !potentials))) return NAVGPU_ERR_INVALID;
  if (!total) return NAVGPU_OK;
  NavfnGuard guard_(h);
  int rc = reserveRos(h);
  if (rc) return rc;
  NavfnRosState& ros = h->ros;
  std::vector<NrCloudPlan> plans(count);
  std::vector<int32_t> qplan;
  qplan.reserve((size_t)total);
  for (uint32_t k = 0; k < count; ++k) {
    plans[k] = NrCloudPlan{frames[3 * k], frames[3 * k + 1], frames[3 * k + 2], 0, h->final_array[first + k]};
    qplan.insert(qplan.end(), query_counts[k], (int32_t)k);
  }
  rc = growBuffer(h, &ros.d_q, &ros.q_cap, (size_t)total * 2);
  if (!rc) rc = growBuffer(h, &ros.d_qplan, &ros.qplan_cap, (size_t)total);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ros.d_cloud_plans, plans.data(), sizeof(NrCloudPlan) * count, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(ros.d_qplan, qplan.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(ros.d_q, points, sizeof(double) * 2 * total, hipMemcpyHostToDevice, h->stream));
  launch_nr_point_potential(h->nv, first, ros.d_cloud_plans, ros.d_qplan, ros.d_q, (uint32_t)total, h->stream);
  std::vector<double> back((size_t)total * 2);
  HIP_TRY(hipMemcpyAsync(back.data(), ros.d_q, sizeof(double) * 2 * total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;
  for (uint64_t q = 0; q < total; ++q) potentials[q] = back[2 * q];
  return NAVGPU_OK;
}

int navgpu_navfn_ros_valid_point_potential(navgpu_navfn* h, uint32_t first, uint32_t count, const double* frames, const uint32_t* query_counts,
                                           const double* points, const double* tolerances, int32_t* flags) {
  if (!h || !frames || !query_counts || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (!framesOk("navgpu_navfn_ros_valid_point_potential", frames, count)) return NAVGPU_ERR_INVALID;
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; ++k) total += query_counts[k];
  if (total > 0x7FFFFFFFu || (total && (!points || !tolerances || !flags))) return NAVGPU_ERR_INVALID;
  if (!total) return NAVGPU_OK;
  std::vector<NrWindow> win;
  win.reserve((size_t)total);
  std::vector<double> seq;
  for (uint32_t k = 0, q = 0; k < count; ++k)
    for (uint32_t i = 0; i < query_counts[k]; ++i, ++q) {
      NrWindow w{};
      w.origin_x = frames[3 * k], w.origin_y = frames[3 * k + 1], w.resolution = frames[3 * k + 2];
      w.goal_x = points[2 * q], w.goal_y = points[2 * q + 1];
      w.plan = k;
      w.seq = (uint32_t)seq.size();
      const int wy = windowSequence(w.goal_y, tolerances[q], w.resolution, seq);
      const int wx = wy < 0 ? -1 : windowSequence(w.goal_x, tolerances[q], w.resolution, seq);
      if (wx < 0 || seq.size() > 0x7FFFFFFFu) {
        g_last_error = "navgpu_navfn_ros_valid_point_potential: more than 4096 window candidates per axis";
        return NAVGPU_ERR_INVALID;
      }
      w.ny = (uint32_t)wy, w.nx = (uint32_t)wx;
      win.push_back(w);
    }
  NavfnGuard guard_(h);
  int rc = reserveRos(h);
  if (rc) return rc;
  NavfnRosState& ros = h->ros;
  for (NrWindow& w : win) w.use_alt = h->final_array[first + w.plan];
  rc = uploadWindows(h, win, seq);
  if (rc) return rc;
  launch_nr_window(h->nv, first, ros.d_win, ros.d_seq, (uint32_t)total, 1, ros.d_best, h->stream);
  std::vector<NrBest> best((size_t)total);
  HIP_TRY(hipMemcpyAsync(best.data(), ros.d_best, sizeof(NrBest) * total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;
  for (uint64_t q = 0; q < total; ++q) flags[q] = best[q].candidates ? 1 : 0;
  return NAVGPU_OK;
}

int navgpu_navfn_ros_potential_cloud(navgpu_navfn* h, uint32_t first, uint32_t count, const double* frames, uint32_t capacity,
                                     navgpu_navfn_ros_cloud_point* points, uint32_t* offsets) {
  if (!h || !frames || !offsets || (!points && capacity) || !navfnRange(h, first, count)) return NAVGPU_ERR_INVALID;
  if (count > 65535 || (uint64_t)count * (uint64_t)h->nv.ns > 0xFFFFFFFFull) return NAVGPU_ERR_INVALID;
  if (!framesOk("navgpu_navfn_ros_potential_cloud", frames, count)) return NAVGPU_ERR_INVALID;
  static_assert(sizeof(NrCloudPoint) == sizeof(navgpu_navfn_ros_cloud_point), "the cloud's point is the header's");
  NavfnGuard guard_(h);
  const NavfnDev& nv = h->nv;
  int rc = reserveRos(h);
  if (rc) return rc;
  NavfnRosState& ros = h->ros;
  std::vector<NrCloudPlan> plans(count);
  for (uint32_t k = 0; k < count; ++k)
    plans[k] = NrCloudPlan{frames[3 * k], frames[3 * k + 1], frames[3 * k + 2], ros.nav_start[first + k], h->final_array[first + k]};
  const uint32_t chunks = navgpu::nrCloudChunks(nv.ns);
  rc = growBuffer(h, &ros.d_totals, &ros.totals_cap, (size_t)chunks * count);
  if (rc) return rc;
  // one device buffer: the offsets (padded to the points' alignment), then room for the points that fit.  Two copies come back:
  // the offsets, then only as many points as they say there are (capacity may be far above that)
  const size_t n_fit = (size_t)std::min<uint64_t>((uint64_t)count * (uint64_t)nv.ns, capacity);
  const size_t off_bytes = ((size_t)(count + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
  rc = growBuffer(h, &ros.d_cloud, &ros.cloud_bytes, off_bytes + n_fit * sizeof(NrCloudPoint));
  if (rc) return rc;
  uint32_t* d_offsets = reinterpret_cast<uint32_t*>(ros.d_cloud);
  NrCloudPoint* d_points = reinterpret_cast<NrCloudPoint*>(ros.d_cloud + off_bytes);
  HIP_TRY(hipMemcpyAsync(ros.d_cloud_plans, plans.data(), sizeof(NrCloudPlan) * count, hipMemcpyHostToDevice, h->stream));
  launch_nr_cloud_count(nv, first, count, ros.d_cloud_plans, ros.d_totals, d_offsets, h->stream);
  if (n_fit) launch_nr_cloud_emit(nv, first, count, ros.d_cloud_plans, ros.d_totals, d_points, (uint32_t)n_fit, h->stream);
  HIP_TRY(hipMemcpyAsync(offsets, d_offsets, sizeof(uint32_t) * (count + 1), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(waitStream(h->stream));
  rc = checkLaunch();
  if (rc) return rc;
  const size_t n_write = std::min<size_t>(offsets[count], n_fit);
  if (n_write) {
    HIP_TRY(hipMemcpyAsync(points, d_points, n_write * sizeof(NrCloudPoint), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(waitStream(h->stream));
  }
  return NAVGPU_OK;
}

}  // extern "C"
