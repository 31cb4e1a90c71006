// k_score (gfx950): generateTrajectory + the six DWA critics, one lane per velocity sample.
// Compiled with -ffp-contract=off: the fp64 step arithmetic on fp32 state has to round exactly
// like the reference (simple_trajectory_generator.cpp:253-260, SURVEY 7 hard part 2).
#include "planner_score.h"

namespace navgpu {

// ------------------------------------------------------------------------------------------------
// k_score: one lane per velocity sample.
//   SimpleTrajectoryGenerator::generateTrajectory / computeNewPositions / computeNewVelocities
//     (simple_trajectory_generator.cpp:180-276)
//   SimpleScoredSamplingPlanner::scoreTrajectory (simple_scored_sampling_planner.cpp:50-79) with the
//     critic order of dwa_planner.cpp:167-173: oscillation, obstacle, goal_front, alignment, path, goal
//   ObstacleCostFunction::scoreTrajectory/footprintCost (obstacle_cost_function.cpp:74-142),
//   WorldModel::footprintCost (world_model.h:65-86), CostmapModel::footprintCost/lineCost/pointCost
//     (costmap_model.cpp:50-142), LineIterator (line_iterator.h:38-139)
//   MapGridCostFunction::scoreTrajectory (map_grid_cost_function.cpp:75-129, aggregation Last)
//   OscillationCostFunction::scoreTrajectory (oscillation_cost_function.cpp:166-176)
// Every sample is scored in full (no early-out against the incumbent): critic terms are
// non-negative, so the first strict minimum is the same sample the reference keeps.
// The costmap window the trajectories can reach is staged in LDS; cells outside it (never needed
// with a correctly sized window) fall back to a global load, so results never depend on it.
// ------------------------------------------------------------------------------------------------
#ifdef NAVGPU_PREP_TIMING  // experiment builds only (tools/probe_prep_timing.py): where k_score_prep_tab's time goes (one workgroup in 16 reports)
__device__ unsigned long long g_prep_stats[16];
#define PREP_STAMP(i) prep_t[i] = wall_clock64()
#else
#define PREP_STAMP(i)
#endif

// ---- stage (k_score_gen*): the footprint and the axis samples, loaded into registers before the image copy
struct ScoreInputs {
  static constexpr int kAxisChunks = (3 * kMaxAxis + kScoreThreads - 1) / kScoreThreads;
  double fp;
  float axis[kAxisChunks];
};
__device__ __forceinline__ ScoreInputs loadInputs(const PlannerDev& pl, const ScoreRobot& r) {
  const uint32_t tid = threadIdx.x;
  ScoreInputs in;
  in.fp = pl.fp_spec[(size_t)r.inst * kMaxFootprint * 2 + (tid < 2 * r.nfp ? tid : 0)];
#pragma unroll
  for (int u = 0; u < ScoreInputs::kAxisChunks; ++u) {
    const uint32_t i = min(tid + (uint32_t)u * kScoreThreads, 3u * kMaxAxis - 1), a = i / kMaxAxis, k = i - a * kMaxAxis;
    in.axis[u] = pl.axis_samples[((size_t)r.inst * 3 + a) * pl.max_axis + min(k, pl.max_axis - 1)];
    if (k >= pl.max_axis) in.axis[u] = 0.f;
  }
  return in;
}
// ---- stage (k_score_gen*): the stored image to LDS, with the footprint / axis samples loadInputs holds; one barrier
__device__ __forceinline__ void loadImage(const PlannerDev& pl, const ScoreRobot& r, const ScoreInputs& in, double* s_fp, float (*s_axis)[kMaxAxis],
                                          uint8_t* s_dyn) {
  const uint32_t tid = threadIdx.x;
  const uint4* img = reinterpret_cast<const uint4*>(pl.prep + (size_t)r.inst * pl.prep_stride);
  uint4* lds = reinterpret_cast<uint4*>(s_dyn);
  const uint32_t n16 = pl.prep_bytes >> 4;
  for (uint32_t i = tid; i < n16; i += blockDim.x) lds[i] = img[i];
  if (tid < 2 * r.nfp) s_fp[tid] = in.fp;
#pragma unroll
  for (int u = 0; u < ScoreInputs::kAxisChunks; ++u) {
    const uint32_t i = tid + (uint32_t)u * kScoreThreads;
    if (i < 3u * kMaxAxis) s_axis[i / kMaxAxis][i % kMaxAxis] = in.axis[u];
  }
  __syncthreads();
}

// ---- stage: one lane per velocity sample - rollout, critics, the sample's outputs - and the workgroup's partial argmin
// CHUNK: cells of a footprint edge fetched per LDS round trip (see planner_score.h); AGG: the general MapGrid step
// TERMS (k_score_terms*, the trajectory cloud's terms pass): the stage stores one SampleTerms record per slot to `terms` and
// NOTHING else - no sample_cost / sample_status, no partial argmin, no counters (the cycle's own scoring launch has written those)
// PROBES (k_check_traj*, with EXPLICIT: every probe is scored as checkTrajectory scores its sample): the robot has n_probes samples at
// `explicit_sample`, three floats each; the lane of slot s reads probe s and stores scoreTrajectory's value to probe_cost[s] and NOTHING
// else, as above - the cycle's result buffers stay the last cycle's
template <bool EXPLICIT, int CHUNK, bool AGG, bool TERMS = false, bool PROBES = false>
__device__ __forceinline__ void scoreSamples(const PlannerDev& pl, const ScoreRobot& r, const double* s_fp, const float (*s_axis)[kMaxAxis],
                                             const uint8_t* s_dyn, double* s_rc, int* s_ri, int* s_cnt, const float* explicit_sample,
                                             SampleTerms* terms = nullptr, uint32_t n_probes = 0, double* probe_cost = nullptr) {
  static_assert(!PROBES || (EXPLICIT && !TERMS), "probes are explicit samples");
  const uint32_t tid = threadIdx.x;
  const navgpu_dwa_config& c = pl.cfg;
  const RobotLimits& lim = pl.limits[r.inst];
  const Geom& g = r.g;
  const navgpu_robot_state& st = r.st;
  const uint8_t* master = r.master;
  const uint32_t *dpath = r.dpath, *dgoal = r.dgoal, *dfront = r.dfront;
  const int32_t* cnt = r.cnt;
  const uint32_t inst = r.inst, nfp = r.nfp;
  const int n_samples = PROBES ? (int)n_probes : EXPLICIT ? 1 : cnt[3];
  const int win = r.win, wx0 = r.wx0, wy0 = r.wy0, win_bytes = r.win_bytes, nw = r.nw;
  const uint8_t* s_win = s_dyn;
  const bool walk_swap = pl.cfg.allow_unknown != 0;  // the window bytes are in walk order (buildScreens)
  const uint32_t walk_fail = walk_swap ? 255u : 254u;
  // NOTE: the LDS read is unconditional (clamped index) and the global fallback sits in its own
  // rarely-taken branch; a `cond ? lds[i] : global[j]` form makes hipcc merge both into one FLAT load.
  auto inWin = [&](int x, int y) { return (unsigned)(x - wx0) < (unsigned)win && (unsigned)(y - wy0) < (unsigned)win; };
  auto cellCost = [&](int x, int y) -> uint8_t {
    const bool in = inWin(x, y);
    uint32_t v = s_win[in ? (y - wy0) * win + (x - wx0) : 0];
    asm volatile("" : "+v"(v));  // pin the ds_read here so it cannot be re-merged with the global load below
    if (walk_swap && v >= 254u) v ^= 1u;  // back from walk order
    if (__builtin_expect(!in, 0)) v = master[y * g.nx + x];
    return (uint8_t)v;
  };
  const double inv_res = pl.inv_res;
  const WorldToMapFast w2m{g, inv_res};
  const uint8_t fail_span = (pl.cfg.allow_unknown != 0) ? 0 : 1;  // pointCost: 254, and 255 unless allow_unknown

  // lane -> sample slot: the slot index (x-outer, y, theta-inner, as the reference enumerates) is what results are keyed by
  const int sidx = blockIdx.x * blockDim.x + tid;
  const bool in_range = sidx < n_samples;
  double total = -1.0;
  int status = NAVGPU_SAMPLE_REJECTED;
  struct NoTerms {};
  [[maybe_unused]] std::conditional_t<TERMS, SampleTerms, NoTerms> rec{};  // (a slot the generator rejects keeps this one)
  if constexpr (TERMS) rec = SampleTerms{{0, 0, 0, 0, 0}, 6, 0, NAVGPU_SAMPLE_REJECTED, 0};

  if (in_range) {
    float vs[3];
    if (EXPLICIT) {
      const float* es = PROBES ? explicit_sample + 3 * (size_t)sidx : explicit_sample;
      vs[0] = es[0];
      vs[1] = es[1];
      vs[2] = es[2];
    } else {
      const int nth = cnt[2], nyv = cnt[1];
      const int ix = sidx / (nyv * nth);
      const int rem = sidx - ix * (nyv * nth);
      const int iy = rem / nth;
      const int ith = rem - iy * nth;
      vs[0] = s_axis[0][ix];
      vs[1] = s_axis[1][iy];
      vs[2] = s_axis[2][ith];
    }
    // ---- generateTrajectory: reject tests and step count (:193-216)
    const double vmag = hyp2((double)vs[0], (double)vs[1]);
    const double eps = 1e-4;
    bool reject = false;
    if ((lim.min_trans_vel >= 0 && vmag + eps < lim.min_trans_vel) && (lim.min_rot_vel >= 0 && fabs((double)vs[2]) + eps < lim.min_rot_vel)) reject = true;
    if (lim.max_trans_vel >= 0 && vmag - eps > lim.max_trans_vel) reject = true;
    int num_steps = 0;
    if (!reject) {
      double ns;
      if (c.discretize_by_time) {
        ns = ceil(c.sim_time / c.sim_granularity);
      } else {
        double sim_time_distance = vmag * c.sim_time;
        double sim_time_angle = fabs((double)vs[2]) * c.sim_time;
        ns = ceil(fmax(sim_time_distance / c.sim_granularity, sim_time_angle / c.angular_sim_granularity));
      }
      num_steps = (int)ns;
      if (num_steps <= 0) reject = true;  // `return num_steps > 0` (:250)
      if (num_steps > (int)pl.max_sim_steps) num_steps = (int)pl.max_sim_steps;  // host validates the capacity
    }
    // DWAPlanner::checkTrajectory ignores generateTrajectory's return value and scores whatever
    // points exist (dwa_planner.cpp:229-230): a rejected sample is an empty trajectory, cost 0.
    if (EXPLICIT && reject) {
      reject = false;
      num_steps = 0;
    }
    if (!reject) {
      status = NAVGPU_SAMPLE_SCORED;
      const double dt = c.sim_time / num_steps;
      const bool continued = !c.use_dwa;
      float px = st.pos[0], py = st.pos[1], pth = st.pos[2];
      float lv[3] = {vs[0], vs[1], vs[2]};
      const float acc[3] = {(float)lim.acc_lim_x, (float)lim.acc_lim_y, (float)lim.acc_lim_theta};
      auto newVel = [&](const float* vel_in, float* out) {  // computeNewVelocities (:265-276)
        for (int i = 0; i < 3; ++i) {
          if (vel_in[i] < vs[i])
            out[i] = (float)fmin((double)vs[i], vel_in[i] + acc[i] * dt);
          else
            out[i] = (float)fmax((double)vs[i], vel_in[i] - acc[i] * dt);
        }
      };
      if (continued) {
        float t0[3];
        newVel(st.vel, t0);
        lv[0] = t0[0];
        lv[1] = t0[1];
        lv[2] = t0[2];
      }
      const double xv = lv[0], yv = lv[1], thv = lv[2];  // traj.xv_, yv_, thetav_

      // ---- critics
      const uint32_t osc = EXPLICIT ? 0u : pl.osc_flags[inst];
      const bool osc_fail = ((osc & NAVGPU_OSC_FORWARD_POS_ONLY) && xv < 0.0) || ((osc & NAVGPU_OSC_FORWARD_NEG_ONLY) && xv > 0.0) ||
                            ((osc & NAVGPU_OSC_STRAFE_POS_ONLY) && yv < 0.0) || ((osc & NAVGPU_OSC_STRAFE_NEG_ONLY) && yv > 0.0) ||
                            ((osc & NAVGPU_OSC_ROT_POS_ONLY) && thv < 0.0) || ((osc & NAVGPU_OSC_ROT_NEG_ONLY) && thv > 0.0);
      const double sc_obs = pl.scale_obstacle, sc_gf = pl.scale_goal, sc_al = pl.align_on[inst] ? pl.scale_path : 0.0,
                   sc_path = pl.scale_path, sc_goal = pl.scale_goal;
      const bool en_obs = sc_obs != 0, en_gf = sc_gf != 0, en_al = sc_al != 0, en_path = sc_path != 0, en_goal = sc_goal != 0;
      double fail_code = 0;  // code of critic `first_fail`: the only one scoreTrajectory's in-order sum can return
      double v_obs = 0, v_gf = 0, v_al = 0, v_path = 0, v_goal = 0;
      if constexpr (AGG) {  // `if (aggregationType_ == Product) cost = 1.0` (:77-79)
        if (pl.mg_agg[0] == 2) v_path = 1.0;
        if (pl.mg_agg[1] == 2) v_goal = 1.0;
        if (pl.mg_agg[2] == 2) v_gf = 1.0;
        if (pl.mg_agg[3] == 2) v_al = 1.0;
      }
      int first_fail = 6;  // order index of the earliest critic that failed (1..5), 6 = none
      const bool allow_unknown = c.allow_unknown != 0;
      const double fpd = c.forward_point_distance;
      const uint32_t N_obst = pl.cells, N_unreach = pl.cells + 1;

      if (en_obs && nfp == 0) {  // "Footprint spec is empty" (obstacle_cost_function.cpp:78-82)
        fail_code = -9.0;
        first_fail = 1;
      }
      // a critic is live while no critic before it in the order has failed; the lowest enabled order decides when
      // nothing is left to evaluate
      const int min_order = en_obs ? 1 : en_gf ? 2 : en_al ? 3 : en_path ? 4 : en_goal ? 5 : 6;
      // the forward point (x + fpd cos, y + fpd sin) stays on the map whenever the centre cell is this many cells
      // away from every border; only then may a step skip its worldToMap
      const uint32_t fwd_margin = (uint32_t)fmin(ceil(fabs(fpd) * inv_res) + 1.0, 1.0e6);
      const bool fwd_screen = !(en_gf || en_al) || (2u * fwd_margin < g.nx && 2u * fwd_margin < g.ny);
      const uint32_t fwd_lo = (en_gf || en_al) ? fwd_margin : 0u, fwd_nx = g.nx - 2u * fwd_lo, fwd_ny = g.ny - 2u * fwd_lo;
      // (the screens' LDS offset in a vector register: as a scalar it is spilled and read back with v_readlane at every point)
      uint32_t fb_off = (uint32_t)win_bytes;
      asm volatile("" : "+v"(fb_off));
      const uint4* s_fb4 = reinterpret_cast<const uint4*>(s_dyn + fb_off);
      // which of the four screens count: obstacle (dilated "not free" with sum_scores, else dilated "can fail"), path, goal
      const bool scr_sum = c.sum_scores != 0;  // the obstacle screen: dilated "not free" with sum_scores, else dilated "can fail"
      const bool screen_on = !AGG && fwd_screen && (nfp >= 3 || !en_obs);
      // the forward-margin test is only needed when the LDS window reaches into the margin band of the map (wave-uniform)
      const bool need_margin = !((uint32_t)wx0 - fwd_lo < fwd_nx && (uint32_t)(wx0 + win - 1) - fwd_lo < fwd_nx && (uint32_t)wy0 - fwd_lo < fwd_ny &&
                                 (uint32_t)(wy0 + win - 1) - fwd_lo < fwd_ny);
      uint32_t scr_z = 0xFFFFFFFFu, scr_w = 0xFFFFFFFFu;  // the path / goal screens count while their critics are live
      if (osc_fail) {
        total = -5.0;
      } else {
        for (int step = 0; step < num_steps; ++step) {
          if (first_fail <= min_order) break;
          const double x = px, y = py, th = pth;
          double sn, cs;
          sincos(th, &sn, &cs);
          uint32_t cx = 0, cy = 0;
          const bool ok_c = w2m(x, y, cx, cy);
          // ---- screen: on every point but the last a critic can only FAIL (its value is overwritten: aggregation
          // Last; with sum_scores the obstacle critic adds the point's cost, which is 0 when everything in reach is
          // free).  One 16-byte LDS read says whether any critic could fail here; if none can, the point is done.
          // Branch-free up to the decision: the screen word is read whatever the point is (clamped address) and the NEXT
          // pose is computed while that read is in flight - the step's LDS round trips used to be waited for one by one,
          // each behind its own exec-mask branch (38 % of the kernel's wave cycles were spent parked, profiles/round3_b).
          const bool in_w = ok_c && inWin((int)cx, (int)cy);
          const int lxw = in_w ? (int)cx - wx0 : 0;
          const uint4 fbw = s_fb4[(in_w ? (int)cy - wy0 : 0) * nw + (lxw >> 5)];
          // ---- advance (computeNewPositions :253-260): fp64 on fp32 state, rounded back to fp32
          if (continued) {
            float t1[3];
            newVel(lv, t1);
            lv[0] = t1[0];
            lv[1] = t1[1];
            lv[2] = t1[2];
          }
          double sn2 = 0.0, cs2 = 0.0;
          if (lv[1] != 0.0f) sincos(M_PI_2 + th, &sn2, &cs2);
          // (rollout_trig 1: cos(pos[2]) names the float function and vel[0] * cos(pos[2]) is a float product - navgpu.h; its value is
          // taken as the double function's, rounded to float)
          const double tx = c.rollout_trig ? (double)(lv[0] * (float)cs) : lv[0] * cs, ty = c.rollout_trig ? (double)(lv[0] * (float)sn) : lv[0] * sn;
          const float nxp = (float)(px + (tx + lv[1] * cs2) * dt);
          const float nyp = (float)(py + (ty + lv[1] * sn2) * dt);
          const float ntp = (float)(pth + lv[2] * dt);
          // (a critic that has already failed, or that follows one that has, cannot change the outcome any more: scr_z / scr_w)
          const uint32_t any = (scr_sum ? fbw.x : fbw.y) | (fbw.z & scr_z) | (fbw.w & scr_w);
          const bool margin_ok = !need_margin || ((cx - fwd_lo < fwd_nx) && (cy - fwd_lo < fwd_ny));
          const bool screened = screen_on && step != num_steps - 1 && in_w && !((any >> (lxw & 31)) & 1u) && margin_ok;
          if (!screened) {
          const bool live_obs = en_obs && 1 < first_fail;
          // all_free: every cell the footprint can touch is FREE_SPACE -> the step costs exactly 0.
          // Without sum_scores only the LAST point's footprint cost survives (obstacle_cost_function.cpp:
          // cost = f_cost), the earlier points only have to be legal: no failing cell in reach is enough.
          bool all_free = false;
          if (live_obs && nfp >= 3 && in_w) {  // (the same screen word as above)
            const bool not_free = (fbw.x >> (lxw & 31)) & 1u, can_fail = (fbw.y >> (lxw & 31)) & 1u;
            all_free = !not_free || (!c.sum_scores && step != num_steps - 1 && !can_fail);
          }
          if (live_obs && all_free) {
            v_obs = c.sum_scores ? v_obs + 0.0 : 0.0;
          } else if (live_obs) {
            double f_cost = 0.0;
            bool bad = !ok_c;  // CostmapModel::footprintCost: centre off the map -> -1
            if (!bad) {
              if (nfp < 3) {
                uint8_t cc = cellCost(cx, cy);
                if (cc == kLethal || cc == kInscribed || (cc == kNoInfo && !allow_unknown))
                  bad = true;
                else
                  f_cost = cc;
              } else {
                int fx0 = 0, fy0 = 0, pxc = 0, pyc = 0;
                uint32_t mx_cost = 0;  // maximum over the perimeter cells, in walk order
                for (uint32_t v = 0; v <= nfp && !bad; ++v) {
                  int vx, vy;
                  if (v < nfp) {
                    const double sx = s_fp[2 * v], sy = s_fp[2 * v + 1];
                    const double wx = x + (sx * cs - sy * sn), wy = y + (sx * sn + sy * cs);
                    uint32_t ux, uy;
                    if (!w2m(wx, wy, ux, uy)) {
                      bad = true;
                      break;
                    }
                    vx = (int)ux;
                    vy = (int)uy;
                    if (v == 0) {
                      fx0 = vx;
                      fy0 = vy;
                      pxc = vx;
                      pyc = vy;
                      continue;
                    }
                  } else {  // closing edge: last -> first
                    vx = fx0;
                    vy = fy0;
                  }
                  // lineCost over LineIterator(pxc, pyc, vx, vy)
                  int deltax = vx - pxc, deltay = vy - pyc;
                  deltax = deltax < 0 ? -deltax : deltax;
                  deltay = deltay < 0 ? -deltay : deltay;
                  int lx = pxc, ly = pyc;
                  int xinc1, xinc2, yinc1, yinc2, den, num, numadd, numpixels;
                  xinc1 = xinc2 = (vx >= pxc) ? 1 : -1;
                  yinc1 = yinc2 = (vy >= pyc) ? 1 : -1;
                  if (deltax >= deltay) {
                    xinc1 = 0;
                    yinc2 = 0;
                    den = deltax;
                    num = deltax / 2;
                    numadd = deltay;
                    numpixels = deltax;
                  } else {
                    xinc2 = 0;
                    yinc1 = 0;
                    den = deltay;
                    num = deltay / 2;
                    numadd = deltax;
                    numpixels = deltay;
                  }
                  if (__builtin_expect(inWin(pxc, pyc) && inWin(vx, vy), 1)) {
                    // every cell of the line lies in the endpoints' bounding box, hence in the window.
                    // The Bresenham addresses do not depend on the bytes read, so the cells are fetched
                    // kChunk at a time with all ds_reads in flight together (one wait per chunk instead
                    // of one dependent LDS round trip per cell); cells past the end re-read the first
                    // cell, cells past a lethal cell cannot change the outcome (-1 either way).
                    constexpr int kChunk = CHUNK;
                    // (the LDS address itself is stepped: with an index, the window's base is added again for every cell)
                    const uint8_t* pw = s_win + ((pyc - wy0) * win + (pxc - wx0));
                    const uint8_t* const pw_first = pw;
                    const int inc1 = yinc1 * win + xinc1, inc2 = yinc2 * win + xinc2;
                    for (int cp = 0; cp <= numpixels && !bad; cp += kChunk) {
                      uint32_t cellv[kChunk];
#pragma unroll
                      for (int u = 0; u < kChunk; ++u) {
                        cellv[u] = *((cp + u <= numpixels) ? pw : pw_first);
                        num += numadd;
                        if (num >= den) {
                          num -= den;
                          pw += inc1;
                        }
                        pw += inc2;
                      }
#pragma unroll
                      for (int u = 0; u < kChunk; ++u) mx_cost = max(mx_cost, cellv[u]);
                      bad = mx_cost >= walk_fail;
                    }
                  } else {
                    for (int cp = 0; cp <= numpixels; ++cp) {
                      const uint8_t cc = master[ly * g.nx + lx];
                      if ((uint8_t)(cc - kLethal) <= fail_span) {
                        bad = true;
                        break;
                      }
                      const uint32_t ct = (walk_swap && cc >= 254) ? (cc ^ 1u) : cc;  // walk order, like the LDS bytes
                      mx_cost = ct > mx_cost ? ct : mx_cost;
                      num += numadd;
                      if (num >= den) {
                        num -= den;
                        lx += xinc1;
                        ly += yinc1;
                      }
                      lx += xinc2;
                      ly += yinc2;
                    }
                  }
                  pxc = vx;
                  pyc = vy;
                }
                f_cost = (walk_swap && mx_cost == 254u) ? 255.0 : (double)mx_cost;  // an allowed NO_INFORMATION cell costs 255
              }
            }
            if (bad) {
              fail_code = -6.0;
              first_fail = 1;
            } else {
              // ok_c holds here, so the -7 branch (obstacle_cost_function.cpp:135-137) cannot fire
              const double occ = fmax(fmax(0.0, f_cost), (double)cellCost(cx, cy));
              v_obs = c.sum_scores ? v_obs + occ : occ;
            }
          }
          if constexpr (AGG) {
            // the general MapGridCostFunction step, critic by critic in the order DWAPlanner lists them
            auto critic = [&](bool en, int order, const uint32_t* grid, double xs, double ys, bool stop_on_failure, int agg, double& v) {
              if (!(en && order < first_fail)) return;
              double sx = x, sy = y;
              if (xs != 0.0) {
                sx = sx + xs * cs;
                sy = sy + xs * sn;
              }
              if (ys != 0.0) {
                double s2, c2;
                sincos(th + M_PI_2, &s2, &c2);
                sx = sx + ys * c2;
                sy = sy + ys * s2;
              }
              uint32_t ux, uy;
              if (!w2m(sx, sy, ux, uy)) {
                fail_code = -4.0;
                first_fail = order;
                return;
              }
              const uint32_t d = grid[uy * g.nx + ux];
              if (stop_on_failure && (d == N_obst || d == N_unreach)) {
                fail_code = d == N_obst ? -3.0 : -2.0;
                first_fail = order;
                return;
              }
              const double gd = (double)d;
              if (agg == 0)
                v = gd;
              else if (agg == 1)
                v += gd;
              else if (v > 0)
                v *= gd;
            };
            critic(en_gf, 2, dfront, fpd, pl.mg_yshift[2], false, pl.mg_agg[2], v_gf);
            critic(en_al, 3, dpath, fpd, pl.mg_yshift[3], false, pl.mg_agg[3], v_al);
            critic(en_path, 4, dpath, 0.0, pl.mg_yshift[0], true, pl.mg_agg[0], v_path);
            critic(en_goal, 5, dgoal, 0.0, pl.mg_yshift[1], true, pl.mg_agg[1], v_goal);
          } else {
          if ((en_path && 4 < first_fail) || (en_goal && 5 < first_fail)) {
            if (!ok_c) {
              if (en_path && 4 < first_fail) {
                fail_code = -4.0;
                first_fail = 4;
              } else {
                fail_code = -4.0;
                first_fail = 5;
              }
            } else {
              const uint32_t cell = cy * g.nx + cx;
              // A point of the window whose path / goal screen bit is clear cannot fail that critic (the bit IS the failure
              // test, taken from this cycle's grid by the prep launch), and of the distances only the LAST point's survives
              // (aggregation Last): no look-up.  Points that leave the screened path because an obstacle is near - most of
              // them - used to wait for two L2 round trips here.
              const bool last_pt = step == num_steps - 1;
              const bool look_p = last_pt || !in_w || ((fbw.z >> (lxw & 31)) & 1u);
              const bool look_g = last_pt || !in_w || ((fbw.w >> (lxw & 31)) & 1u);
              if (en_path && 4 < first_fail && look_p) {
                const uint32_t d = dpath[cell];
                if (d == N_obst) {
                  fail_code = -3.0;
                  first_fail = 4;
                } else if (d == N_unreach) {
                  fail_code = -2.0;
                  first_fail = 4;
                } else
                  v_path = d;
              }
              if (en_goal && 5 < first_fail && look_g) {
                const uint32_t d = dgoal[cell];
                if (d == N_obst) {
                  fail_code = -3.0;
                  first_fail = 5;
                } else if (d == N_unreach) {
                  fail_code = -2.0;
                  first_fail = 5;
                } else
                  v_goal = d;
              }
            }
          }
          if ((en_gf && 2 < first_fail) || (en_al && 3 < first_fail)) {
            double sx = x, sy = y;
            if (fpd != 0.0) {
              sx = x + fpd * cs;
              sy = y + fpd * sn;
            }
            uint32_t ux, uy;
            if (!w2m(sx, sy, ux, uy)) {
              if (en_gf && 2 < first_fail) {
                fail_code = -4.0;
                first_fail = 2;
              } else {
                fail_code = -4.0;
                first_fail = 3;
              }
            } else if (step == num_steps - 1) {  // aggregation Last: only the final point's value survives
              const uint32_t cell = uy * g.nx + ux;
              if (en_gf && 2 < first_fail) v_gf = dfront[cell];
              if (en_al && 3 < first_fail) v_al = dpath[cell];
            }
          }
          }  // !AGG
          scr_z = first_fail > 4 ? 0xFFFFFFFFu : 0u;  // (first_fail only changes in here)
          scr_w = first_fail > 5 ? 0xFFFFFFFFu : 0u;
          }  // !screened
          px = nxp;
          py = nyp;
          pth = ntp;
        }
        // ---- scoreTrajectory sum in critic order
        // (the first failing critic in that order ends the sum with its code: simple_scored_sampling_planner.cpp:59-66)
        total = 0.0;
        if (first_fail < 6) {
          total = fail_code;
        } else {
          addCritic(total, en_obs, v_obs, sc_obs);
          addCritic(total, en_gf, v_gf, sc_gf);
          addCritic(total, en_al, v_al, sc_al);
          addCritic(total, en_path, v_path, sc_path);
          addCritic(total, en_goal, v_goal, sc_goal);
        }
      }
      if constexpr (TERMS) {  // the raw critic values in critic order; the oscillation critic fails as order 0
        rec = SampleTerms{{v_obs, v_gf, v_al, v_path, v_goal}, osc_fail ? 0 : first_fail, osc_fail ? -5 : (int32_t)fail_code, status, num_steps};
      }
    }
    if constexpr (TERMS) {
      terms[sidx] = rec;
    } else if constexpr (PROBES) {
      probe_cost[sidx] = total;
    } else if (!EXPLICIT && pl.sample_cost) {
      pl.sample_cost[(size_t)inst * pl.max_samples + sidx] = total;
      pl.sample_status[(size_t)inst * pl.max_samples + sidx] = status;
    }
  }
  if constexpr (TERMS || PROBES) return;

  // ---- workgroup argmin (lowest index wins ties == first strict minimum of the sequential loop)
  const bool valid = in_range && status == NAVGPU_SAMPLE_SCORED && total >= 0.0;
  double bc = valid ? total : 1.0e300;
  int bi = valid ? sidx : 0x7FFFFFFF;
  for (int off = 32; off > 0; off >>= 1) {
    double oc = __shfl_down(bc, off);
    int oi = __shfl_down(bi, off);
    if (oc < bc || (oc == bc && oi < bi)) {
      bc = oc;
      bi = oi;
    }
  }
  const unsigned long long m_scored = __ballot(in_range && status == NAVGPU_SAMPLE_SCORED);
  const unsigned long long m_valid = __ballot(valid);
  if ((tid & 63) == 0) {
    s_rc[tid >> 6] = bc;
    s_ri[tid >> 6] = bi;
    atomicAdd(&s_cnt[0], __popcll(m_scored));
    atomicAdd(&s_cnt[1], __popcll(m_valid));
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kScoreThreads / 64; ++w)
      if (s_rc[w] < bc || (s_rc[w] == bc && s_ri[w] < bi)) {
        bc = s_rc[w];
        bi = s_ri[w];
      }
    pl.part_cost[(size_t)inst * pl.score_blocks + blockIdx.x] = bc;  // score_blocks = capacity (256-thread blocks)
    pl.part_index[(size_t)inst * pl.score_blocks + blockIdx.x] = bi;
    if (s_cnt[0]) atomicAdd(&pl.counters[2 * inst], s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&pl.counters[2 * inst + 1], s_cnt[1]);
  }
}

constexpr int kScorePrepThreads = NAVGPU_SCORE_PREP_THREADS;  // the workgroup that builds a robot's image

// k_score_prep_tab: a robot's image with the heading tables, and what k_score_sweep reads behind it
template <class Robots>
__global__ __launch_bounds__(kScorePrepThreads) void k_score_prep_tab(PlannerDev pl, Robots robots) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ double s_fp[2 * kMaxFootprint];
  __shared__ float s_axis[3][kMaxAxis];
  __shared__ int s_cnt[2];
#ifdef NAVGPU_PREP_TIMING
  unsigned long long prep_t[6];
#endif
  PREP_STAMP(0);
  ScoreRobot r = scoreRobot(pl, robots(blockIdx.y));
  const SweepLimits lim = sweepLimits(pl, r.inst);
  stageInputs<false>(pl, r, s_fp, s_axis, s_cnt, s_dyn);
  __syncthreads();
  PREP_STAMP(1);
  buildScreens(pl, r, s_dyn, reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes + score_bits_bytes(r.win) + pl.tab_bytes));
  PREP_STAMP(2);
  buildTables(pl, r, s_fp, s_axis, s_dyn);
  __syncthreads();
  PREP_STAMP(3);
  storeImage(pl, r, s_dyn);
  PREP_STAMP(4);
  storeSweepScalars(pl, r, s_axis, s_cnt, s_dyn, lim);
#ifdef NAVGPU_PREP_TIMING
  PREP_STAMP(5);
  if (threadIdx.x == 0 && (blockIdx.y & 15u) == 3u) {
    for (int i = 0; i < 5; ++i) atomicAdd(&g_prep_stats[i], prep_t[i + 1] - prep_t[i]);
    atomicAdd(&g_prep_stats[15], 1ull);
  }
#endif
}
// k_score_prep_grids: completes the image scorePrepFree stored (the prep workgroups of the wavefront launch) once the path and goal
// grids stand: words 2 and 3 of every screen cell, the free distance and start_fail (aux[7], aux[8]).  No other byte of the image
// changes.  Latency bound, so every load it needs is issued before the first is waited for: STEPS covers the padded window.
template <int STEPS, class Robots>
__global__ __launch_bounds__(kScorePrepThreads) void k_score_prep_grids(PlannerDev pl, Robots robots) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ int s_min;
  ScoreRobot r = scoreRobot(pl, robots(blockIdx.y));
  placeWindow(r);
  uint32_t* s_fb = reinterpret_cast<uint32_t*>(s_dyn);  // [win][nw][4]
  uint4* img = reinterpret_cast<uint4*>(pl.prep + (size_t)r.inst * pl.prep_stride + r.win_bytes);
  const int n = r.win * r.nw;
  // words 0 and 1 come back from the stored image: the first of a lane is in flight with the grid loads
  const uint4 v0 = img[min((int)threadIdx.x, n - 1)];
  buildGridScreens<STEPS>(pl, r, s_fb);
  if ((int)threadIdx.x < n) {
    s_fb[4 * threadIdx.x] = v0.x;
    s_fb[4 * threadIdx.x + 1] = v0.y;
  }
  for (int it = threadIdx.x + blockDim.x; it < n; it += blockDim.x) {
    const uint4 v = img[it];
    s_fb[4 * it] = v.x;
    s_fb[4 * it + 1] = v.y;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < n; it += blockDim.x) *reinterpret_cast<uint2*>(&img[it].z) = make_uint2(s_fb[4 * it + 2], s_fb[4 * it + 3]);
  storeFreeDistance(pl, r, s_fb, &s_min);
}
// k_score_prep_gen: a robot's image (window and screens) for the k_score_gen* workgroups
// (Plain kernels around one body, not a template like the others: the statics of a kernel template have vague linkage, and the
// compiler then keeps the 2 KB of s_fp / s_axis that this kernel stages and never reads - as a plain kernel it drops them.)
template <class Robots>
__device__ __forceinline__ void scorePrepGen(const PlannerDev& pl, Robots robots, double* s_fp, float (*s_axis)[kMaxAxis], int* s_cnt) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  ScoreRobot r = scoreRobot(pl, robots(blockIdx.y));
  stageInputs<false>(pl, r, s_fp, s_axis, s_cnt, s_dyn);
  __syncthreads();
  buildScreens(pl, r, s_dyn, reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes + score_bits_bytes(r.win)));
  __syncthreads();
  storeImage(pl, r, s_dyn);
}
__global__ __launch_bounds__(kScoreThreads) void k_score_prep_gen(PlannerDev pl, RobotRange robots) {
  __shared__ double s_fp[2 * kMaxFootprint];
  __shared__ float s_axis[3][kMaxAxis];
  __shared__ int s_cnt[2];
  scorePrepGen(pl, robots, s_fp, s_axis, s_cnt);
}
__global__ __launch_bounds__(kScoreThreads) void k_score_prep_gen_list(PlannerDev pl, RobotList robots) {
  __shared__ double s_fp[2 * kMaxFootprint];
  __shared__ float s_axis[3][kMaxAxis];
  __shared__ int s_cnt[2];
  scorePrepGen(pl, robots, s_fp, s_axis, s_cnt);
}
static auto prepGenKernel(RobotRange) { return k_score_prep_gen; }
static auto prepGenKernel(RobotList) { return k_score_prep_gen_list; }
// k_score_gen<CHUNK> / k_score_gen_agg: the samples of a robot, from the image k_score_prep_gen stored
template <int CHUNK, bool AGG, bool TERMS = false, class Robots>
__device__ __forceinline__ void scoreGen(const PlannerDev& pl, Robots robots, SampleTerms* terms = nullptr) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ double s_fp[2 * kMaxFootprint];
  __shared__ float s_axis[3][kMaxAxis];
  __shared__ double s_rc[kScoreThreads / 64];
  __shared__ int s_ri[kScoreThreads / 64];
  __shared__ int s_cnt[2];
  // A scoring workgroup's prologue (a few dependent loads, the image copy, barriers) is a handful of instructions, but its
  // waves are the YOUNGEST on their SIMDs and lose every issue arbitration against the five older workgroups in their
  // rollout loops: measured 40 % of a workgroup's residence before its first trajectory point.  Raised priority until the
  // image is in place gets it out of the way.
  __builtin_amdgcn_s_setprio(3);
  ScoreRobot r = scoreRobot(pl, robots(blockIdx.y));
  // The footprint and axis samples stay in registers until the image is copied, and go to LDS with it: ONE batch of
  // loads in flight and one barrier instead of five dependent round trips and three barriers (a load takes several
  // microseconds while 24 waves per CU gather from the distance grids).
  const ScoreInputs in = loadInputs(pl, r);
  if (threadIdx.x == 0) s_cnt[0] = s_cnt[1] = 0;
  placeWindow(r);
  loadImage(pl, r, in, s_fp, s_axis, s_dyn);
  __builtin_amdgcn_s_setprio(0);
  scoreSamples<false, CHUNK, AGG, TERMS>(pl, r, s_fp, s_axis, s_dyn, s_rc, s_ri, s_cnt, nullptr, terms);
}
// k_score_explicit(_agg): checkTrajectory's one sample, on an image built in the workgroup itself
template <bool AGG>
__device__ __forceinline__ void scoreExplicit(const PlannerDev& pl, uint32_t first, const float* explicit_sample) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ double s_fp[2 * kMaxFootprint];
  __shared__ float s_axis[3][kMaxAxis];
  __shared__ double s_rc[kScoreThreads / 64];
  __shared__ int s_ri[kScoreThreads / 64];
  __shared__ int s_cnt[2];
  ScoreRobot r = scoreRobot(pl, first + blockIdx.y);
  stageInputs<true>(pl, r, s_fp, s_axis, s_cnt, s_dyn);
  __syncthreads();
  buildScreens(pl, r, s_dyn, reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes + score_bits_bytes(r.win)));
  __syncthreads();
  scoreSamples<true, 12, AGG>(pl, r, s_fp, s_axis, s_dyn, s_rc, s_ri, s_cnt, explicit_sample);
}
template <int CHUNK, class Robots>
__global__ __launch_bounds__(kScoreThreads) void k_score_gen(PlannerDev pl, Robots robots, const float* explicit_sample) {
  scoreGen<CHUNK, false>(pl, robots);
}
template <class Robots>
__global__ __launch_bounds__(kScoreThreads) void k_score_gen_agg(PlannerDev pl, Robots robots, const float* explicit_sample) {
  scoreGen<16, true>(pl, robots);
}
__global__ __launch_bounds__(kScoreThreads) void k_score_explicit(PlannerDev pl, uint32_t first, const float* explicit_sample) {
  scoreExplicit<false>(pl, first, explicit_sample);
}
__global__ __launch_bounds__(kScoreThreads) void k_score_explicit_agg(PlannerDev pl, uint32_t first, const float* explicit_sample) {
  scoreExplicit<true>(pl, first, explicit_sample);
}
// k_check_traj(_agg): checkTrajectory for the robots of a list, each with a run of probes (navgpu_planner_check_trajectories).
// blockIdx.y = position in the list, blockIdx.x = block of kScoreThreads probes of that robot: the workgroup builds the robot's image as
// scoreExplicit does, then scores one probe per lane.  A robot with fewer probes than the launch's widest has workgroups with
// nothing to do: they leave before the first barrier.  The oscillation flags of a robot with probes are cleared here
// (dwa_planner.cpp:217; no probe reads them: an explicit sample is scored against cleared flags).
template <bool AGG>
__device__ __forceinline__ void checkTraj(const PlannerDev& pl, const ProbeBatch& pb) {
  extern __shared__ __align__(16) uint8_t s_dyn[];
  __shared__ double s_fp[2 * kMaxFootprint];
  __shared__ float s_axis[3][kMaxAxis];
  __shared__ int s_cnt[2];
  const uint32_t p0 = pb.offsets[blockIdx.y], n = pb.offsets[blockIdx.y + 1] - p0;
  if (blockIdx.x * kScoreThreads >= n) return;  // (the same for every lane of the workgroup)
  ScoreRobot r = scoreRobot(pl, pb.instances[blockIdx.y]);
  if (blockIdx.x == 0 && threadIdx.x == 0) pl.osc_flags[r.inst] = 0;
  stageInputs<true>(pl, r, s_fp, s_axis, s_cnt, s_dyn);
  __syncthreads();
  buildScreens(pl, r, s_dyn, reinterpret_cast<uint32_t*>(s_dyn + r.win_bytes + score_bits_bytes(r.win)));
  __syncthreads();
  scoreSamples<true, 12, AGG, false, true>(pl, r, s_fp, s_axis, s_dyn, nullptr, nullptr, s_cnt, pb.vel + 3 * (size_t)p0, nullptr, n, pb.cost + p0);
}
__global__ __launch_bounds__(kScoreThreads) void k_check_traj(PlannerDev pl, ProbeBatch pb) { checkTraj<false>(pl, pb); }
__global__ __launch_bounds__(kScoreThreads) void k_check_traj_agg(PlannerDev pl, ProbeBatch pb) { checkTraj<true>(pl, pb); }

// k_score_terms / k_score_terms_agg (the trajectory cloud's terms pass, navgpu_planner_set_trajectory_cloud): the general stage with
// TERMS set, for ONE robot whose records go to `terms` [max_samples].  The footprint chunk only groups LDS reads (the
// critic values do not depend on it), so one instantiation serves every footprint.
__global__ __launch_bounds__(kScoreThreads) void k_score_terms(PlannerDev pl, uint32_t inst, SampleTerms* terms) {
  scoreGen<16, false, true>(pl, RobotRange{inst}, terms);
}
__global__ __launch_bounds__(kScoreThreads) void k_score_terms_agg(PlannerDev pl, uint32_t inst, SampleTerms* terms) {
  scoreGen<16, true, true>(pl, RobotRange{inst}, terms);
}

size_t score_window_bytes(uint32_t win) {  // costmap window + the four per-cell screens
  return (((size_t)win * win + 15) & ~(size_t)15) + score_bits_bytes((int)win);
}
size_t score_table_row_bytes(const PlannerDev& pl) { return (size_t)pl.tab_steps * ((4 + 2 * pl.tab_nfp) * sizeof(double) + sizeof(float)); }
size_t score_table_bytes(const PlannerDev& pl) {  // all v_theta rows: the image k_score_prep_tab builds
  return ((size_t)pl.tab_nth * score_table_row_bytes(pl) + 15) & ~(size_t)15;
}
size_t score_table_lds_bytes(const PlannerDev& pl) {  // the tab_rows rows of one row group: what a k_score_sweep workgroup holds
  return ((size_t)pl.tab_rows * score_table_row_bytes(pl) + 15) & ~(size_t)15;
}
// v_theta rows per row group and the LDS budget they were sized for; 0 = no tables.  A workgroup's image (window +
// screens + rows) should leave room for three workgroups per CU (52 KB each), else two (78 KB); the image of ALL
// rows has to fit the one workgroup that builds it.
uint32_t score_table_rows(const PlannerDev& pl, uint32_t win) {
  const size_t wb = score_window_bytes(win), row = score_table_row_bytes(pl);
  if (row == 0 || wb + score_table_bytes(pl) + score_scratch_bytes((int)win) > 150u * 1024u) return 0;
  for (size_t budget : {(size_t)NAVGPU_SCORE_TAB_LDS_KB * 1024, (size_t)52 * 1024, (size_t)78 * 1024}) {
    if (wb + 16 >= budget) continue;
    const size_t r = (budget - wb - 16) / row;
    if (r >= 1) return (uint32_t)std::min<size_t>(r, pl.tab_nth);
  }
  return 0;
}
size_t score_prep_bytes(const PlannerDev& pl) {  // the LDS image k_score_prep* stores per robot
  return score_window_bytes(pl.win) + (pl.use_tables ? score_table_bytes(pl) : 0);
}
size_t score_prep_slot_bytes(const PlannerDev& pl) {  // a robot's slot of pl.prep: the image, the sweep launch's scalars, the pairs' reject bytes
  return ((score_prep_bytes(pl) + 255) & ~(size_t)255) + kScoreAuxBytes + score_prep_reject_bytes(pl);
}
size_t score_prep_free_lds_bytes(const PlannerDev& pl) {
  return score_window_bytes(pl.win) + pl.tab_bytes + score_scratch_bytes((int)pl.win) + score_prep_free_tail_bytes();
}
void score_prep_tab_sizes(PlannerDev& pl) {
  // the prep workgroup builds all table rows (its LDS holds the whole image); a sweep workgroup loads one row group
  pl.tab_bytes = (uint32_t)score_table_bytes(pl);
  pl.prep_bytes = (uint32_t)score_prep_bytes(pl);
}
static uint32_t sweepLaunch(const PlannerDev& pl, RobotRange r, uint32_t count, hipStream_t s) { return launch_score_sweep(pl, r.first, count, s); }
static uint32_t sweepLaunch(const PlannerDev& pl, RobotList r, uint32_t count, hipStream_t s) { return launch_score_sweep_list(pl, r.list, count, s); }
// a cycle's scoring launches for the robots of a range or a list
template <class Robots>
static uint32_t launchScoreCycle(const PlannerDev& pl_in, Robots robots, uint32_t count, hipStream_t s, bool grids_only = false) {
  PlannerDev pl = pl_in;
  const size_t win_bytes = score_window_bytes(pl.win);
  const size_t scratch = score_scratch_bytes((int)pl.win);  // only where the image is built
  if (score_sweep_applies(pl)) {
    score_prep_tab_sizes(pl);
    if (grids_only) {  // the wavefront launch's prep workgroups have stored the rest of the image (launch_bfs_prep)
      const uint32_t steps = ((uint32_t)pl.win * ((pl.win + 31) & ~31u) + kScorePrepThreads - 1) / kScorePrepThreads;
      auto grids = steps <= 8 ? k_score_prep_grids<8, Robots> : (steps <= 16 ? k_score_prep_grids<16, Robots> : k_score_prep_grids<32, Robots>);
      launchScore(grids, dim3(1, count), kScorePrepThreads, score_bits_bytes((int)pl.win), s, pl, robots);
    } else {
      launchScore(k_score_prep_tab<Robots>, dim3(1, count), kScorePrepThreads, win_bytes + score_table_bytes(pl) + scratch, s, pl, robots);
    }
    return sweepLaunch(pl, robots, count, s);
  }
  // the general path (no tables, or mg_generic: the general step has no table variant)
  pl.use_tables = 0;
  pl.prep_bytes = (uint32_t)score_prep_bytes(pl);
  const uint32_t gen_blocks = (pl.max_samples + kScoreThreads - 1) / kScoreThreads;  // (score_blocks is the capacity of the partial results)
  launchScore(prepGenKernel(robots), dim3(1, count), kScoreThreads, win_bytes + scratch, s, pl, robots);
  auto gen = pl.mg_generic        ? k_score_gen_agg<Robots>
             : pl.fp_chunk <= 6  ? k_score_gen<6, Robots>
             : pl.fp_chunk <= 9  ? k_score_gen<9, Robots>
             : pl.fp_chunk <= 12 ? k_score_gen<12, Robots>
                                 : k_score_gen<16, Robots>;
  launchScore(gen, dim3(gen_blocks, count), kScoreThreads, win_bytes, s, pl, robots, (const float*)nullptr);
  return gen_blocks;
}
uint32_t launch_score(const PlannerDev& pl, uint32_t first, uint32_t count, const float* explicit_sample, hipStream_t s) {
  if (explicit_sample) {
    const size_t lds = score_window_bytes(pl.win) + score_scratch_bytes((int)pl.win);
    launchScore(pl.mg_generic ? k_score_explicit_agg : k_score_explicit, dim3(1, count), kScoreThreads, lds, s, pl, first, explicit_sample);
    return 1;
  }
  return launchScoreCycle(pl, RobotRange{first}, count, s);
}
uint32_t launch_score_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s) { return launchScoreCycle(pl, RobotList{list}, count, s); }
// the scoring launches behind a wavefront launch with prep workgroups (split_prep_applies): k_score_prep_grids in k_score_prep_tab's place
uint32_t launch_score_grids(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s) { return launchScoreCycle(pl, RobotRange{first}, count, s, true); }
uint32_t launch_score_grids_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s) {
  return launchScoreCycle(pl, RobotList{list}, count, s, true);
}

// The probes of n_robots listed robots in one launch; max_probes: the longest run of the list (> 0).  The image is built in the
// workgroup, so the dynamic LDS is k_score_explicit's.
void launch_check_traj(const PlannerDev& pl, const ProbeBatch& pb, uint32_t n_robots, uint32_t max_probes, hipStream_t s) {
  const size_t lds = score_window_bytes(pl.win) + score_scratch_bytes((int)pl.win);
  launchScore(pl.mg_generic ? k_check_traj_agg : k_check_traj, dim3((max_probes + kScoreThreads - 1) / kScoreThreads, n_robots), kScoreThreads, lds, s, pl, pb);
}

// The terms pass of one robot, behind the cycle's scoring launch: its image is rebuilt in its slot of pl.prep in the general
// kernels' form (a table configuration's image has been consumed by k_score_sweep by now), then every slot is scored again
// into `terms`.
void launch_score_terms(const PlannerDev& pl_in, uint32_t inst, SampleTerms* terms, hipStream_t s) {
  PlannerDev pl = pl_in;
  const size_t win_bytes = score_window_bytes(pl.win);
  pl.use_tables = 0;
  pl.prep_bytes = (uint32_t)score_prep_bytes(pl);
  const uint32_t gen_blocks = (pl.max_samples + kScoreThreads - 1) / kScoreThreads;
  launchScore(k_score_prep_gen, dim3(1, 1), kScoreThreads, win_bytes + score_scratch_bytes((int)pl.win), s, pl, RobotRange{inst});
  launchScore(pl.mg_generic ? k_score_terms_agg : k_score_terms, dim3(gen_blocks, 1), kScoreThreads, win_bytes, s, pl, inst, terms);
}

#ifdef NAVGPU_PREP_TIMING
extern "C" int navgpu_debug_prep_stats(unsigned long long* out16, int reset) {
  if (out16) hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_prep_stats), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(g_prep_stats), z, sizeof(z));
  }
  return 0;
}
#endif

}  // namespace navgpu
