// Internal header shared by the HIP kernels and the C-ABI host code (gfx950 only).
// Data layout in HBM (all SoA over instances, instance-major):
//   master/static/obstacle : uint8  [n][cells_padded]   row-major, index = my*size_x + mx
//   voxel                  : uint32 [n][cells_padded]
//   path / goal / goal_front: uint32 [n][cells]   MapGrid target_dist of path_costs_ (shared by
//                            alignment_costs_, same target poses), goal_costs_, goal_front_costs_
// MapGrid distances are stored as uint32 (the reference keeps doubles that only ever hold
// integers <= size_x*size_y+1; map_cell.h:44-64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/navgpu.h"

namespace navgpu {

constexpr uint8_t kNoInfo = 255, kLethal = 254, kInscribed = 253, kFree = 0;
constexpr int kMaxFootprint = 32;
constexpr int kCareRows = 128, kCareWords = 4;  // bounded wavefronts: extent of the per-robot pocket mask (k_samples)
constexpr uint32_t kSeedListMax = 1024;         // wavefront seed lists: entries allocated per (robot, grid) (k_samples)
constexpr uint32_t kNoSeedList = 0xFFFFFFFFu;   // ... a list's count when its cells did not fit: that wavefront seeds from the plan
#ifndef NAVGPU_SCORE_TAB_THREADS
#define NAVGPU_SCORE_TAB_THREADS 256  // samples per k_score_sweep workgroup (as for round 2's table kernel - 512 with a 52 KB image: 0.523 ms; 256 with 26 KB: 0.516 ms, configs[4] 2.17 -> 1.82 ms)
#endif
#ifndef NAVGPU_SCORE_TAB_LDS_KB
#define NAVGPU_SCORE_TAB_LDS_KB 14    // first LDS budget score_table_rows tries for a k_score_sweep workgroup's image (window + screens + its row group's table rows): 3 v_theta rows at configs[2] (round 2's table kernel, 26 KB = 9 rows: 0.526 -> 0.506 ms)
#endif
#ifndef NAVGPU_SCORE_PREP_THREADS
#define NAVGPU_SCORE_PREP_THREADS 256  // threads of the workgroup that builds a robot's image (k_score_prep_*): alone 512 is 3 us faster, but beside the other stream groups' kernels its 8 waves and 53 KB wait longer for a CU (0.872 -> 0.862 ms per step)
#endif
#ifndef NAVGPU_SCORE_THREADS
#define NAVGPU_SCORE_THREADS 256
#endif
// A/B and trace switches read from the environment exist in tool builds only (make EXTRA=-DNAVGPU_DEBUG_SWITCHES, tools/):
// the library that is loaded into move_base reads no environment variable.
#ifdef NAVGPU_DEBUG_SWITCHES
#define NAVGPU_DEBUG_ENV(name) getenv(name)
#else
#define NAVGPU_DEBUG_ENV(name) ((const char*)nullptr)
#endif
constexpr int kScoreThreads = NAVGPU_SCORE_THREADS;  // samples per k_score workgroup  // vertices kept in registers/LDS by the kernels

// Which robot block or work item k of a launch belongs to: the k-th of a contiguous range (navgpu_planner_cycle, navgpu_costmap_update)
// or of a strictly increasing list in device memory (navgpu_planner_cycle_list, navgpu_costmap_update_list).  Every kernel of the
// planner cycle and of the costmap update is a template over one of the two, one copy of its body.  RobotRange has the size and
// alignment of the `uint32_t first` it stands for: the range instantiations take the argument block, and compile to the code, they
// had as plain kernels.
struct RobotRange {
  uint32_t first;
  __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return first + k; }
  __device__ __forceinline__ uint32_t front() const { return first; }
};
struct RobotList {
  const uint32_t* list;
  __device__ __forceinline__ uint32_t operator()(uint32_t k) const { return list[k]; }
  __device__ __forceinline__ uint32_t front() const { return list[0]; }
};
static_assert(sizeof(RobotRange) == sizeof(uint32_t) && alignof(RobotRange) == alignof(uint32_t), "the range kernels' argument block");

struct InstCostmapState {  // per-instance state that persists across update cycles (device resident)
  double last_min_x, last_min_y, last_max_x, last_max_y;  // InflationLayer::last_* (inflation_layer.cpp:63-66)
  int32_t need_reinflation;                               // InflationLayer::need_reinflation_
  int32_t static_has_updated_data;                        // StaticLayer::has_updated_data_
  int32_t box[4];                                         // x0, xn, y0, yn of the last updateMap
  int32_t box_valid;                                      // 0 when xn < x0 || yn < y0 (layered_costmap.cpp:128-135)
  int32_t pad;
  double bounds[4];                                       // min_x, min_y, max_x, max_y after all updateBounds
  double extra[4];                                        // CostmapLayer::extra_min_x_, _min_y_, _max_x_, _max_y_ of the obstacle layer
  int32_t has_extra_bounds, pad2;                         // (costmap_layer.cpp:21-60)
};

struct ObsCsr {  // one observation, device form
  uint32_t first_point, n_points, flags, pad;
  double ox, oy, oz;
  double obstacle_range, raytrace_range;
};

// CellData of inflation_layer.h:55-80 as the heap stores it: the key is the RANK of distance_ among the distinct cached
// distances (same order, same ties), the source a signed offset from the cell (x_, y_ follow from index_)
struct PqCell {
  uint32_t index;
  uint16_t rank;
  int8_t sdx, sdy;
};
static_assert(sizeof(PqCell) == 8, "heap entry");
struct CostmapDev {
  uint32_t nx, ny, cells, cells_padded;
  double res;
  int32_t layers, track_unknown;
  uint8_t master_default, obstacle_default;
  // layer params
  int32_t obs_enabled, footprint_clearing, combination_method, static_use_maximum, static_received;
  double max_obstacle_height;
  // voxel
  int32_t z_voxels, unknown_threshold, mark_threshold;
  double origin_z, z_resolution;
  // inflation
  int32_t infl_enabled;
  uint32_t R;  // cell_inflation_radius_
  double inflation_radius;
  // buffers
  double* origin;      // [n][2]
  uint8_t *master, *stat, *obst;
  uint32_t* voxel;
  uint8_t* lut;        // (R+2)^2 cost table with 0 where cached distance > R
  uint8_t* lut2;       // [256] cost by squared cell distance (k_inflate_bits), valid when lut2_ok
  int32_t lut2_ok;
  // reference-order mode (navgpu_inflation_params::priority_queue_order): InflationLayer's own priority-queue walk
  int32_t infl_pq;
  double* dist_lut;    // (R+2)^2 uint16 ranks of cached_distances_ = hypot(i, j) (host libm) among their distinct values; 0xFFFF beyond the radius
  uint8_t* pq_seen;    // [n][cells] seen_
  PqCell* pq_heap;     // [n][pq_cap] the binary heap std::priority_queue<CellData> keeps
  uint64_t pq_cap;
  // StaticLayer of a rolling-window costmap: one static map with its own geometry, a transform per robot
  uint8_t* stat_roll;   // [stat_ny][stat_nx] interpreted costs (nullptr: not a rolling static layer / no map yet)
  uint32_t stat_nx, stat_ny;
  double stat_res, stat_ox, stat_oy;
  double* stat_tf;      // [n][12] tf::Transform map_frame <- global_frame: basis row-major, origin
  InstCostmapState* state;  // [n]
  // staged cycle inputs
  double* pose;        // [n][3]
  double* fp_world;    // [n][kMaxFootprint][2] transformed footprint (host fp64 libm, footprint.cpp:103-118)
  uint32_t* fp_n;      // [n]
  ObsCsr* obs;         // [n][max_obs] observations of the staged cycle (first_point relative to the instance block)
  uint32_t* obs_count; // [n]
  float* points;       // [n][max_points][3] xyz
  uint32_t max_obs, max_points;
  int32_t* shift;      // [n][2] pending rolling-window shift in cells (cell_ox, cell_oy)
  uint8_t *master_alt, *obst_alt;  // ping-pong targets of the shift
  uint32_t* voxel_alt;
  uint2* mark_seq;     // [n][max_points] voxel marking with mark_threshold > 0: (cell, valid | column bits before marking | z) in point order
};

// One robot's planner half of base_local_planner::LocalPlannerLimits (local_planner_limits.h:47-57): the eleven velocity and
// acceleration limits, the leading fields of navgpu_dwa_config and of navgpu_robot_limits in their order.  PlannerDev::limits holds
// one per instance; every kernel reads its robot's record where it used to read these fields of pl.cfg (whose copies are what
// navgpu_planner_configure wrote last, for the legacy planner and the tools).
struct RobotLimits {
  double max_trans_vel, min_trans_vel;
  double max_vel_x, min_vel_x, max_vel_y, min_vel_y;
  double max_rot_vel, min_rot_vel;
  double acc_lim_x, acc_lim_y, acc_lim_theta;
};
static_assert(sizeof(RobotLimits) == 88, "eleven doubles, as they lead navgpu_dwa_config and navgpu_robot_limits");

struct PlannerDev {
  uint32_t nx, ny, cells;
  double res, inv_res;
  double* origin;  // [n][2] (shared with the costmap)
  const uint8_t* master;
  uint32_t cells_padded;
  navgpu_dwa_config cfg;
  RobotLimits* limits;        // [n] per-robot limits (navgpu_planner_set_limits; navgpu_planner_configure writes cfg's into every record)
  // derived once per configure (dwa_planner.cpp:64-75)
  double scale_path, scale_goal, scale_obstacle;
  uint32_t max_plan, max_sim_steps, max_axis;  // max_axis = per-axis sample capacity
  uint32_t max_samples, score_blocks;
  // staged inputs
  navgpu_robot_state* state;  // [n]
  double* plan;               // [n][max_plan][2]
  uint32_t* plan_count;       // [n]
  double* front_last;         // [n][2] last pose of front_global_plan (nose goal)
  int32_t* align_on;          // [n] alignment_costs_ scale != 0
  double* fp_spec;            // [n][kMaxFootprint][2] robot-frame footprint
  uint32_t* fp_n;             // [n]
  // per-cycle work buffers
  float* axis_samples;        // [n][3][max_axis]
  int32_t* axis_count;        // [n][4]  (nx, ny, nth, total)
  uint32_t *path, *goal, *goal_front;  // [n][cells] each
  uint32_t* bfs_scratch;      // k_bfs_global bitmaps (only for grids too large for LDS)
  int32_t* bfs_box;           // [n][8] x0, x1, y0, y1 (cells, inclusive) of the robot's region = box of its MapGrid look-ups + 2 cells; x1 < x0 = none; [4] = bfs_care valid (k_samples)
  uint32_t* bfs_care;         // [n][kCareRows][kCareWords] box cells outside pockets, by region row and word from the region's first
  uint32_t* bfs_reach;        // [n] staged half edge of that box in cells, 0 = search the whole grid
  uint32_t bfs_bounded;       // launch switch: stop a wavefront once its robot's box is settled
  unsigned long long* bfs_trace;  // [items][8] wall-clock stamps of the phases of every wavefront (NAVGPU_DEBUG_BFS_TRACE=<file>, tools/trace_bfs.py), else null
  uint32_t* bfs_next_item;    // work counters of the persistent launches: [0] k_bfs_rows2, [1] k_bfs_rows
  uint32_t* bfs_free;         // [n][ny][W] traversable-cell bitmap of the costmaps (k_free_bits, per launch_bfs)
  uint32_t* bfs_levels;       // [n][3] levels the last wavefront of (robot, grid) ran: predicts the next one's length
  uint32_t* bfs_order;        // [n * 3] items of a launch sorted longest first, stored at first * 3 (k_samples)
  uint32_t* bfs_seed_cells;   // [n][3][kSeedListMax] seed cells of (robot, grid) as row * 32 * (words per bitmap row) + column: bitmap word << 5 | bit (k_samples)
  uint32_t* bfs_seed_count;   // [n][3] entries of each list, or kNoSeedList
  uint32_t bfs_seed_cap;      // launch switch: 0 = every wavefront seeds from the plan itself, else k_samples fills the lists with up to that many cells
  uint32_t bfs_grids;         // wavefronts per robot: 3 (DWA: path, goal, goal_front) or 2 (legacy TrajectoryPlanner)
  uint32_t* within;           // legacy planner: [n][ny][W] MapCell::within_robot bits of path_map_ on entry to launch_bfs, whose k_free_bits ORs the costmap's free bits in (= path_map_'s traversable-cell bitmap); else null
  uint32_t win;               // edge (cells) of the costmap window staged in LDS by k_score
  uint32_t fp_rcells;         // Chebyshev radius (cells) that contains every footprint cell around the centre cell
  uint8_t fp_halfw[32];       // by |dy| <= fp_rcells: the largest |dx| at which a footprint cell can lie dy rows from the centre cell (a disc, planWindow); 0xFF: no such row
  uint32_t fp_chunk;          // cells of the longest footprint edge (+1): picks the k_score<CHUNK> instantiation
  uint32_t use_tables, tab_steps, tab_nfp, tab_nth;  // use_tables (planWindow): the prep image carries the heading tables and k_score_sweep scores
  // MapGridCostFunction options beyond DWAPlanner's own wiring (navgpu_planner_set_map_grid_options), indexed
  // 0 path, 1 goal, 2 goal_front, 3 alignment: aggregation 0 Last | 1 Sum | 2 Product, sideways shift in metres
  int32_t mg_agg[4];
  double mg_yshift[4];
  int32_t mg_generic;         // any of them set: the scoring launches take the general step (scoreSamples<..., AGG>)
  uint32_t tab_rows;          // v_theta rows per row group = rows of the tables a k_score_sweep workgroup keeps in LDS
  uint32_t tab_bytes;         // score_table_bytes(): the tables' share of the image k_score_prep_tab builds (set by launch_score for that launch)
  double tab_dt;              // sim_time / tab_steps
  uint8_t* prep;              // [n][prep_stride] LDS image of k_score (window, reach bitmaps, heading tables), built per cycle by k_score_prep*
  uint32_t prep_stride, prep_bytes;
  double* sample_cost;        // [n][max_samples] or null
  int32_t* sample_status;     // [n][max_samples] or null
  double* part_cost;          // [n][score_blocks]
  int32_t* part_index;        // [n][score_blocks]
  int32_t* counters;          // [n][2] scored, valid
  uint32_t* osc_flags;        // [n]
  float* osc_prev;            // [n][3]
  navgpu_plan_result* result; // [n]
  double* traj;               // [n][max_sim_steps][3]
};

// trajectory cloud (navgpu_planner_set_trajectory_cloud): what the terms pass keeps of one sample slot
struct SampleTerms {
  double v[5];         // raw (unscaled) values of the obstacle, goal_front, alignment, path and goal critics
  int32_t first_fail;  // order of the first failing critic: 0 oscillation, 1..5 as above, 6 none
  int32_t fail_code;   // its (negative) code
  int32_t status;      // NAVGPU_SAMPLE_*
  int32_t n_points;    // points of the trajectory (0: rejected by the generator)
};
static_assert(sizeof(SampleTerms) == 56, "terms record");
// per-launch view of one enabled robot (traj_cloud_kernels.hip)
struct TrajCloudDev {
  const SampleTerms* terms;   // [max_samples]
  navgpu_sample_terms* out;   // [max_samples] what k_traj_scan derives per slot
  uint32_t* totals;           // [2] points of the cloud, sample slots
  float* points;              // [capacity][7] or null
  uint32_t capacity;          // points `points` holds
  uint32_t slots_per_group;   // consecutive slots of a k_traj_emit workgroup
  double scale[5];            // the critics' scales at the cycle (alignment: 0 when switched off)
  int32_t reference_costs;
};
void launch_score_terms(const PlannerDev& pl, uint32_t inst, SampleTerms* terms, hipStream_t s);
// batched checkTrajectory (navgpu_planner_check_trajectories): per-launch view of the fleet's probe buffers
struct ProbeBatch {
  const uint32_t* instances;  // [n_robots] absolute robot indices, strictly increasing
  const uint32_t* offsets;    // [n_robots + 1] robot k owns probes offsets[k] .. offsets[k + 1]
  const float* vel;           // [probes][3] velocity samples
  double* cost;               // [probes] scoreTrajectory's value: the weighted sum, or the first failing critic's code
};
// Weak: navgpu_planner_check_trajectories sits beside the single call in navgpu_host.cpp, and that translation unit is also linked
// against a stand-in for the kernels that knows the launchers of its day (tests/tsan); there the call answers NAVGPU_ERR_STATE.
// libnavgpu.so always carries the launcher (planner_score.hip).
__attribute__((weak)) void launch_check_traj(const PlannerDev& pl, const ProbeBatch& pb, uint32_t n_robots, uint32_t max_probes, hipStream_t s);
void launch_traj_scan(const PlannerDev& pl, const TrajCloudDev& t, uint32_t inst, hipStream_t s);
void launch_traj_emit(const PlannerDev& pl, const TrajCloudDev& t, uint32_t inst, uint32_t n_slots, hipStream_t s);
uint32_t traj_emit_slots_per_group(uint32_t max_sim_steps);  // 0: a trajectory of that many points does not fit a workgroup's LDS

// legacy TrajectoryPlanner (tp_kernels.hip)
struct TpOut {  // per generateTrajectory call
  double cost;
  double ex, ey, eth;  // Trajectory::getEndpoint
  double ahead;        // goal_map_ at the heading_lookahead point of the endpoint
  int32_t n_points;
  int32_t ahead_ok;    // that point is on the map
};
struct TpDev {
  navgpu_tp_config cfg;
  uint32_t max_samples;   // capacity per robot
  double* samples;        // [n][max_samples][3] vx, vy, vtheta
  uint32_t* n_samples;    // [n]
  double* start;          // [n][6] x, y, theta, vx, vy, vtheta (fp64 promotions of the Vector3f)
  TpOut* out;             // [n][max_samples]
  int32_t* winner;        // [n] sample whose points k_tp_rollout stores (second pass), -1 none
  double* points;         // [n][max_sim_steps][3]
  uint32_t* within_cells; // [n][max_within] cell indices under the robot
  uint32_t* within_count; // [n]
  uint32_t max_within;
  uint32_t* within_bits;  // [n][ny][W]
};
void launch_tp_within(const PlannerDev& pl, const TpDev& tp, uint32_t first, uint32_t count, hipStream_t s);
void launch_tp_rollout(const PlannerDev& pl, const TpDev& tp, uint32_t first, uint32_t count, int store_points, hipStream_t s);
// ---- the legacy planner for a robot list (navgpu_tp_update_plans_list, navgpu_tp_find_best_path_list): robot k of a launch is
// list[k], a device array, strictly increasing.  One robot's record of the packed upload; the block holds the records, then the plan
// points in use (x, y), then the samples in use (vx, vy, vtheta), then the cells under the robots.
struct TpStageRec {
  double start[6];                  // x, y, theta, vx, vy, vtheta
  uint32_t inst;                    // the robot
  uint32_t n_plan, plan_off;        // plan points and the first of them among the packed points
  uint32_t n_samples, samples_off;  // samples and the first of them among the packed samples (and among the packed results coming back)
  uint32_t n_within, within_off;    // cells under the robot and the first of them among the packed cells
  uint32_t pad;
};
static_assert(sizeof(TpStageRec) == 80, "staged as an array of these in front of the plan points");
struct TpStageBlock {  // per-launch view of the block on the device
  const TpStageRec* rec;
  const double *plan, *samples;
  const uint32_t* within;
};
// Weak for the reason launch_tp_probe (below) is; without them the listed calls answer NAVGPU_ERR_STATE.
__attribute__((weak)) void launch_tp_stage_scatter(const PlannerDev& pl, const TpDev& tp, const TpStageBlock& b, uint32_t n_robots, int with_rollout, hipStream_t s);
__attribute__((weak)) void launch_tp_within_list(const PlannerDev& pl, const TpDev& tp, const uint32_t* list, uint32_t count, hipStream_t s);
__attribute__((weak)) void launch_tp_rollout_list(const PlannerDev& pl, const TpDev& tp, const uint32_t* list, uint32_t count, int store_points, hipStream_t s);
__attribute__((weak)) void launch_tp_gather_out(const TpDev& tp, const TpStageRec* rec, TpOut* packed, uint32_t n_robots, hipStream_t s);
__attribute__((weak)) void launch_tp_winner_scatter(const TpDev& tp, const uint32_t* list, const int32_t* winners, uint32_t n_robots, hipStream_t s);
// batched scoreTrajectory (navgpu_tp_score_trajectories, tp_probe_kernels.hip): per-launch view of the fleet's probe buffers
struct TpProbeBatch {
  const double* probes;      // [n_probes][9] pose x y theta, velocity x y theta, sample x y theta
  const uint32_t* instance;  // [n_probes] the robot a probe belongs to
  double* cost;              // [n_probes] what scoreTrajectory returns
  uint32_t n_probes;
};
// Weak for the reason launch_check_traj is: navgpu_tp.cpp is also linked against a stand-in for the kernels that knows the launchers
// of its day (tests/tsan); there navgpu_tp_score_trajectories answers NAVGPU_ERR_STATE.  libnavgpu.so always carries the launcher.
__attribute__((weak)) void launch_tp_probe(const PlannerDev& pl, const TpDev& tp, const TpProbeBatch& pb, hipStream_t s);

// batched CostmapModel::footprintCost queries (footprint_kernels.hip): runs of poses per robot of a launch, packed
struct FootprintDev {
  uint32_t nx, ny, cells_padded;
  double res;
  const double* origin;     // [n][2]
  const uint8_t* master;    // [n][cells_padded]
  const double* fp_spec;    // [n][kMaxFootprint][2] robot-frame footprint (navgpu_set_footprint)
  const uint32_t* fp_n;     // [n]
  const uint32_t* q_off;    // [count + 1] first query of robot first + k in poses / costs
  const double* poses;      // [queries][3] x, y, theta in the world frame
  double* costs;            // [queries]
  uint32_t* first_hit;      // [count] preset to 0xFFFFFFFF (= -1): the robot's first query that fails (seek_legal: that is legal); or null
  int32_t allow_unknown, seek_legal;
};
void launch_footprint_cost(const FootprintDev& d, uint32_t first, uint32_t count, const uint32_t* h_counts, const uint32_t* h_fp_n, hipStream_t s);

// voxel-layer debug outputs (voxel_export_kernels.hip): per-launch view of the fleet's export scratch
struct VoxelExportDev {
  uint32_t* totals;      // [count][stride] per-chunk totals of launch (a), their exclusive prefix after (b)
  uint32_t stride;
  uint32_t* counts;      // [count]
  uint32_t* obs_counts;  // [count][max_obs] (clearing endpoints)
  void* xyz;             // [count][capacity][3] float or double, or null while counting
  uint32_t capacity;     // points per robot in xyz
  int32_t status, as_double;  // NAVGPU_VOXEL_UNKNOWN / _MARKED; doubles instead of floats (voxel points)
};
constexpr uint32_t kVxThreads = 256;                    // lanes of every export workgroup
constexpr uint32_t kVxPerLane = 4;                      // consecutive columns of a lane: one 16-byte load
constexpr uint32_t kVxChunk = kVxThreads * kVxPerLane;  // columns of a chunk (1000 x 1000: 977 chunks)
constexpr uint32_t kClearChunk = kVxThreads;            // points of a chunk: one per lane (the predicate is ~40 fp64 operations)
inline uint32_t voxel_export_chunks(uint32_t cells) { return (cells + kVxChunk - 1) / kVxChunk; }                  // chunk totals per robot: voxel points
inline uint32_t clear_export_chunks(uint32_t max_points) { return (max_points + kClearChunk - 1) / kClearChunk; }  // ... per observation: clearing endpoints
void launch_voxel_points_count(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s);
void launch_voxel_points_emit(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s);
void launch_clear_endpoints_count(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s);
void launch_clear_endpoints_emit(const CostmapDev& cm, const VoxelExportDev& v, uint32_t first, uint32_t count, hipStream_t s);

// observation buffer (obs_buffer_kernels.hip): the device-resident rings behind navgpu_obsbuf_*
struct ObsIngestCloud {  // one cloud of a navgpu_obsbuf_buffer call that is still in its list when the call returns
  uint32_t kind, first, n, slot;  // NAVGPU_CLOUD_*; into the call's points / ranges; ring slot ((robot * sources + source) * slots + s)
  float m[12];                    // global <- cloud frame, narrowed: basis row-major, origin
  double min_h, max_h;            // the source's height filter
  float angle_min, angle_increment, range_min, range_max;
  int32_t inf_is_valid, pad;
};
static_assert(sizeof(ObsIngestCloud) == 104, "ingest descriptor");
struct ObsRetransform {  // one kept slot of navgpu_obsbuf_set_global_frame
  uint32_t slot, pad;
  float m[12];
};
struct ObsBufDev {
  float* ring;            // [n][sources][slots][max_cloud_points][3] global-frame points that passed the height filter, cloud order
  uint32_t* counts;       // [n][sources][slots] points of a slot
  uint32_t max_cloud_points, slots_per_robot;  // slots_per_robot = sources * slots
};
void launch_obs_ingest(const ObsBufDev& ob, const ObsIngestCloud* clouds, uint32_t n_clouds, const float* points, const float* ranges, hipStream_t s);
void launch_obs_gather(const ObsBufDev& ob, const CostmapDev& cm, uint32_t first, uint32_t count, hipStream_t s);
void launch_obs_retransform(const ObsBufDev& ob, const ObsRetransform* items, uint32_t n_items, hipStream_t s);

// ---- launchers (defined in the .hip files) ---------------------------------------------------
void launch_obstacle(const CostmapDev& cm, uint32_t first, uint32_t count, const double* bounds_in, int only_bounds,
                     hipStream_t s);
void launch_reset_window(uint8_t* grid, size_t stride, uint32_t count, uint32_t nx, uint32_t x0, uint32_t y0, uint32_t xn, uint32_t yn, uint8_t value, hipStream_t s);
void launch_reset_bounding_box(const CostmapDev& cm, uint32_t first, uint32_t count, const double* boxes_world, hipStream_t s);
void launch_merge(const CostmapDev& cm, uint32_t first, uint32_t count, const int32_t* boxes, hipStream_t s, bool layer_only = false);
void launch_inflate(const CostmapDev& cm, uint32_t first, uint32_t count, const int32_t* boxes, hipStream_t s);
void launch_static_interpret(uint8_t* dst, const int8_t* occ, uint32_t cells, uint32_t cells_padded, uint32_t count,
                             int track_unknown_space, int trinary, int lethal_threshold, int unknown_cost_value, hipStream_t s);
void launch_export_window(const uint8_t* master, uint32_t nx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int8_t* out, hipStream_t s);
void launch_fill_u8(uint8_t* dst, uint8_t v, size_t n, hipStream_t s);
void launch_fill_u32(uint32_t* dst, uint32_t v, size_t n, hipStream_t s);
void launch_shift_u8(const uint8_t* src, uint8_t* dst, const CostmapDev& cm, uint32_t first, uint32_t count, uint8_t fill, hipStream_t s);
void launch_shift_u32(const uint32_t* src, uint32_t* dst, const CostmapDev& cm, uint32_t first, uint32_t count, uint32_t fill, hipStream_t s);
// ---- the costmap update for a robot list (navgpu_costmap_*_list): robot k of a launch is robots.list[k], a device array, strictly
// increasing; arrays indexed by block (bounds_in, boxes) stay indexed by list position
void launch_obstacle(const CostmapDev& cm, RobotList robots, uint32_t count, const double* bounds_in, int only_bounds, hipStream_t s);
void launch_merge(const CostmapDev& cm, RobotList robots, uint32_t count, const int32_t* boxes, hipStream_t s, bool layer_only = false);
void launch_inflate(const CostmapDev& cm, RobotList robots, uint32_t count, const int32_t* boxes, hipStream_t s);
void launch_shift_u8(const uint8_t* src, uint8_t* dst, const CostmapDev& cm, RobotList robots, uint32_t count, uint8_t fill, hipStream_t s);
void launch_shift_u32(const uint32_t* src, uint32_t* dst, const CostmapDev& cm, RobotList robots, uint32_t count, uint32_t fill, hipStream_t s);
// a rolling fleet's listed update: the listed robots' shifted grids from the ping-pong target back into place (the fleet-wide
// pointers stay where they are, the unlisted robots' grids untouched)
void launch_shift_back_u8(const uint8_t* alt, uint8_t* grid, const CostmapDev& cm, RobotList robots, uint32_t count, hipStream_t s);
void launch_shift_back_u32(const uint32_t* alt, uint32_t* grid, const CostmapDev& cm, RobotList robots, uint32_t count, hipStream_t s);
void launch_obs_gather(const ObsBufDev& ob, const CostmapDev& cm, RobotList robots, uint32_t count, hipStream_t s);
// navgpu_costmap_stage_list / navgpu_obsbuf_stage_list: one robot's record of the packed upload.  The block holds the records, then the
// world footprints' vertices in use, then the observation descriptors in use, then (navgpu_costmap_stage_list) the points in use.
struct CmStageRec {
  double pose[3];
  double origin[2];   // rolling window: the robot's new origin
  int32_t shift[2];   // ... and its pending shift in cells
  uint32_t inst;      // the robot
  uint32_t fp_n, fp_off;        // footprint vertices and the first of them among the packed vertices
  uint32_t obs_count, obs_off;  // observations and the first of them among the packed descriptors
  uint32_t n_points, pts_off;   // points in use and the first of them among the packed points (0, 0: they stay on the device)
  uint32_t pad;
};
static_assert(sizeof(CmStageRec) == 80, "staged as an array of these in front of the vertices");
void launch_cm_stage_scatter(const CostmapDev& cm, const CmStageRec* rec, const double* fp, const ObsCsr* obs, const float* points, int rolling,
                             uint32_t n_robots, hipStream_t s);

void launch_cell_costs(const PlannerDev& pl, uint32_t inst, float4* out, hipStream_t s);
void launch_samples(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s);
void launch_bfs(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s, const uint32_t* order = nullptr, bool free_ready = false);
uint32_t launch_score(const PlannerDev& pl, uint32_t first, uint32_t count, const float* explicit_sample, hipStream_t s);  // returns blocks per instance
void launch_select(const PlannerDev& pl, uint32_t first, uint32_t count, uint32_t n_blocks, hipStream_t s);
// the poses of up to 64 robots as one kernel-argument block (< 4 KB)
constexpr uint32_t kPoseChunk = 64;
struct PoseChunk {
  navgpu_robot_state* state;  // device arrays, indexed by absolute instance
  double* front_last;
  int32_t* align_on;
  uint32_t* bfs_reach;
  uint32_t first, count;
  navgpu_robot_state st[kPoseChunk];
  double front[2 * kPoseChunk];
  int32_t align[kPoseChunk];
  uint32_t reach[kPoseChunk];
};
static_assert(sizeof(PoseChunk) <= 4096, "kernel arguments are limited to 4 KB");
void launch_stage_poses(const PoseChunk& c, hipStream_t s);
// the limits records of up to 40 robots as one kernel-argument block, for the reason the poses travel that way (k_set_limits).
// Weak as the list launchers below are; without it navgpu_planner_set_limits answers NAVGPU_ERR_STATE.
constexpr uint32_t kLimitsChunk = 40;
struct LimitsChunk {
  RobotLimits* limits;  // the device table, indexed by absolute instance
  uint32_t count, pad;
  uint32_t inst[kLimitsChunk];
  RobotLimits rec[kLimitsChunk];
};
static_assert(sizeof(LimitsChunk) <= 4096, "kernel arguments are limited to 4 KB");
__attribute__((weak)) void launch_set_limits(const LimitsChunk& c, hipStream_t s);
// ---- the cycle for a robot list (navgpu_planner_*_list): robot k of a launch is list[k], a device array, strictly increasing.
// Weak for the reason launch_check_traj is: navgpu_host.cpp is also linked against a stand-in for the kernels that knows the
// launchers of its day (tests/tsan); there the listed calls answer NAVGPU_ERR_STATE.  libnavgpu.so always carries the launchers.
struct PoseChunkList : PoseChunk {  // `first` unused: entry li belongs to robot inst[li]
  uint32_t inst[kPoseChunk];
};
static_assert(sizeof(PoseChunkList) <= 4096, "kernel arguments are limited to 4 KB");
struct StageRec {  // navgpu_planner_stage_list's record of one robot, as uploaded
  navgpu_robot_state st;
  double front[2];    // nose goal
  int32_t align;      // alignment switch
  uint32_t reach;     // wavefront box half edge
  uint32_t inst;      // the robot
  uint32_t plan_off;  // its first pose among the upload's packed poses
};
static_assert(sizeof(StageRec) == 64, "staged as an array of these in front of the poses");
__attribute__((weak)) void launch_stage_poses_list(const PoseChunkList& c, hipStream_t s);
__attribute__((weak)) void launch_stage_scatter(const PlannerDev& pl, const StageRec* rec, const double* poses, uint32_t n_robots, hipStream_t s);
__attribute__((weak)) void launch_samples_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s);
__attribute__((weak)) void launch_bfs_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s, const uint32_t* order = nullptr,
                                           bool free_ready = false);  // as launch_bfs: false = k_free_bits and the work counters are this launch's
__attribute__((weak)) uint32_t launch_score_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s);  // returns blocks per instance
__attribute__((weak)) void launch_select_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, uint32_t n_blocks, hipStream_t s);
// ---- the split image build (navgpu_planner_set_split_prep): the wavefront launch with scorePrepFree workgroups, and the scoring
// launches that complete the image (k_score_prep_grids) where launch_score builds it whole.  Weak as the list launchers are.
__attribute__((weak)) bool split_prep_applies(const PlannerDev& pl);  // the sweep scores and the wavefronts are k_bfs_rows'
__attribute__((weak)) void launch_bfs_prep(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s, const uint32_t* order);
__attribute__((weak)) void launch_bfs_prep_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s, const uint32_t* order);
__attribute__((weak)) uint32_t launch_score_grids(const PlannerDev& pl, uint32_t first, uint32_t count, hipStream_t s);
__attribute__((weak)) uint32_t launch_score_grids_list(const PlannerDev& pl, const uint32_t* list, uint32_t count, hipStream_t s);
void launch_sincos(const double* th, uint32_t n, double* sn, double* cs, hipStream_t s);
// ---- device-resident global plans (local_plan_kernels.hip): LocalPlannerUtil::getLocalPlan per robot and cycle
constexpr uint32_t kPlanWindowThreads = 256;
constexpr uint32_t kPwActive = 1u, kPwTransform = 2u, kPwPrune = 4u;
struct PlanWindowIn {   // what a cycle hands k_plan_window for one robot; every transcendental was taken on the host (libm)
  double pose[2];       // the robot in the global frame
  double robot[2];      // the robot in the plan's frame (tf.transformPose, goal_functions.cpp:113-114)
  double c, sn, tx, ty, tyaw;  // plan -> global: cos / sin of its yaw, translation, yaw
  uint32_t start, len;  // the live part of the robot's slot
  uint32_t flags;       // kPw*
  uint32_t pad;
};
struct PlanWindowRec {  // what it leaves: the public record, the local plan's last point, getGoalPose
  navgpu_local_window w;
  double last[2];
  double goal[3];
};
static_assert(sizeof(PlanWindowIn) == 88 && sizeof(PlanWindowRec) == 64, "staged as arrays of these");
// robots [first, first+count): in / rec are indexed by absolute instance, store is [n][max_global_plan]
void launch_plan_window(const PlannerDev& pl, const navgpu_global_pose* store, uint32_t max_global_plan, uint32_t first, uint32_t count,
                        const PlanWindowIn* in, PlanWindowRec* rec, double sq_dist_threshold, hipStream_t s);
// slot k of the store takes poses[offsets[k] .. offsets[k + 1]) (navgpu_local_planner_set_plans' one upload, scattered)
void launch_plan_scatter(const navgpu_global_pose* poses, const uint32_t* offsets, uint32_t count, navgpu_global_pose* slots,
                         uint32_t max_global_plan, hipStream_t s);
// ---- move_base's plan handover and polygon writes (move_base_kernels.hip)
constexpr uint32_t kPlanPreferThreads = 256;  // sampled poses (every fourth of the plan) a workgroup looks at per chunk
constexpr uint32_t kPpActive = 1u;
constexpr uint32_t kPpNoWrite = 0xFFFFFFFFu;  // an emit offset at or beyond any capacity (a uint32_t): k_gp_plan_emit leaves at once for that plan
struct PlanPreferIn {    // what a handover hands k_plan_prefer for one robot
  double x, y;           // the robot in the plan's frame
  uint32_t stored;       // poses in the robot's slot from its beginning (erased prefix + live part); 0: no resident plan
  uint32_t dropped;      // leading poses of the plan as handed over that a store resize lost
  uint32_t new_len;      // latest_plan_->size()
  uint32_t flags;        // kPpActive: the new plan was made and fits the store
};
static_assert(sizeof(PlanPreferIn) == 32 && sizeof(navgpu_handover_record) == 32, "staged as arrays of these");
// robots [first, first+count): in / rec / emit_off are indexed from 0, persistence by absolute instance, store is [n][max_global_plan].
// emit_off[k] = the robot's slot offset where the decision is ADOPT, kPpNoWrite otherwise.
void launch_plan_prefer(const navgpu_global_pose* store, uint32_t max_global_plan, uint32_t first, uint32_t count, const PlanPreferIn* in,
                        int64_t* persistence, int64_t now_ns, int64_t timeout_ns, navgpu_handover_record* rec, uint32_t* emit_off, hipStream_t s);
// polygon k = xy[off[k] .. off[k + 1]) into grid[(first + k) * stride ...]; ok[k] as Costmap2D::setConvexPolygonCost returns
void launch_set_polygon_cost(const CostmapDev& cm, uint8_t* grid, uint32_t first, uint32_t count, const double* xy, const uint32_t* off,
                             uint8_t value, int32_t* ok, hipStream_t s);
size_t score_table_bytes(const PlannerDev& pl);
size_t score_window_bytes(uint32_t win);
size_t score_prep_bytes(const PlannerDev& pl);
size_t score_prep_slot_bytes(const PlannerDev& pl);
size_t bfs_scratch_words(uint32_t nx, uint32_t ny);
uint32_t score_table_rows(const PlannerDev& pl, uint32_t win);

// ---- device helpers ---------------------------------------------------------------------------
struct Geom {
  double ox, oy, res;
  uint32_t nx, ny;
};

// Costmap2D::worldToMap (costmap_2d.cpp:208-220).  The explicit NaN / range guards reproduce what
// the x86 `(int)double` conversion yields for out-of-range values (0x80000000 -> "not in map").
__device__ __forceinline__ bool worldToMap(const Geom& g, double wx, double wy, uint32_t& mx, uint32_t& my) {
  if (wx < g.ox || wy < g.oy) return false;
  double fx = (wx - g.ox) / g.res;
  double fy = (wy - g.oy) / g.res;
  if (!(fx < 2147483648.0) || !(fy < 2147483648.0)) return false;
  mx = (uint32_t)(int)fx;
  my = (uint32_t)(int)fy;
  return mx < g.nx && my < g.ny;
}

// Costmap2D::raytraceLine + bresenham2D (costmap_2d.h:359-417): `at(offset)` on every visited cell
template <class F>
__device__ __forceinline__ void raytrace2d(uint32_t nx, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t max_length,
                                           F&& at) {
  int dx = (int)x1 - (int)x0, dy = (int)y1 - (int)y0;
  uint32_t abs_dx = dx < 0 ? -dx : dx, abs_dy = dy < 0 ? -dy : dy;
  int offset_dx = dx > 0 ? 1 : -1;  // sign(0) == -1 (costmap_2d.h:414-417)
  int offset_dy = (dy > 0 ? 1 : -1) * (int)nx;
  uint32_t offset = y0 * nx + x0;
  double dist = sqrt((double)dx * (double)dx + (double)dy * (double)dy);  // exact integers: == hypot(dx, dy)
  double scale = (dist == 0.0) ? 1.0 : fmin(1.0, (double)max_length / dist);
  uint32_t abs_da, abs_db, lim;
  int offset_a, offset_b;
  if (abs_dx >= abs_dy) {
    abs_da = abs_dx;
    abs_db = abs_dy;
    offset_a = offset_dx;
    offset_b = offset_dy;
  } else {
    abs_da = abs_dy;
    abs_db = abs_dx;
    offset_a = offset_dy;
    offset_b = offset_dx;
  }
  lim = (uint32_t)(scale * abs_da);
  int error_b = abs_da / 2;
  uint32_t end = lim < abs_da ? lim : abs_da;
  for (uint32_t i = 0; i < end; ++i) {
    at(offset);
    offset += offset_a;
    error_b += abs_db;
    if ((uint32_t)error_b >= abs_da) {
      offset += offset_b;
      error_b -= abs_da;
    }
  }
  at(offset);
}

// |(x, y)| for generic doubles: sqrt of the correctly summed squares (within 1 ulp of libm hypot)
__device__ __forceinline__ double hyp2(double x, double y) {
  double a = x * x, b = y * y;
  double s = a + b;
  double h = sqrt(s);
  if (h == 0.0) return 0.0;
  double bb = s - a;
  double e = (a - (s - bb)) + (b - bb);
  double r = __builtin_fma(-h, h, s);
  return h + (r + e) / (2.0 * h);
}

// VoxelLayer::raytraceFreespace (voxel_layer.cpp:266-372) without the ray walk: what an observation fixes, and the clipped
// end of one point's ray.  k_obstacle<true> walks the ray to that end, k_clear_count / k_clear_emit (voxel_export_kernels.hip)
// return the end itself (the clearing_endpoints cloud); fp64 in the reference's statement order, -ffp-contract=off.
struct VoxelRay {
  double ox, oy, oz;                    // sensor origin
  double sensor_x, sensor_y, sensor_z;  // the same in cells (worldToMap3DFloat, voxel_layer.h:107-118)
  double map_end_x, map_end_y;          // origin + getSizeInMetersX / Y
};
// false: the observation clears nothing (no points, :269-270; sensor origin off the map, :277-284).  size_z = min(z_voxels, 16)
__device__ __forceinline__ bool voxelRayBegin(const Geom& g, const CostmapDev& cm, uint32_t size_z, const ObsCsr& obs, VoxelRay& r) {
  if (obs.n_points == 0) return false;
  r.ox = obs.ox;
  r.oy = obs.oy;
  r.oz = obs.oz;
  if (r.ox < g.ox || r.oy < g.oy || r.oz < cm.origin_z) return false;
  r.sensor_x = (r.ox - g.ox) / g.res;
  r.sensor_y = (r.oy - g.oy) / g.res;
  r.sensor_z = (r.oz - cm.origin_z) / cm.z_resolution;
  if (!(r.sensor_x < g.nx && r.sensor_y < g.ny && r.sensor_z < size_z)) return false;
  r.map_end_x = g.ox + (g.nx - 1 + 0.5) * g.res;
  r.map_end_y = g.oy + (g.ny - 1 + 0.5) * g.res;
  return true;
}
// :297-353 for the point pt[0..2]: (wpx, wpy, wpz) the clipped end in the world, (px, py, pz) in cells; false when it fails
// worldToMap3DFloat at :353 (no ray, no endpoint)
__device__ __forceinline__ bool voxelRayEnd(const Geom& g, const CostmapDev& cm, uint32_t size_z, const VoxelRay& r, const float* pt, double& wpx,
                                            double& wpy, double& wpz, double& px, double& py, double& pz) {
  const double ox = r.ox, oy = r.oy, oz = r.oz;
  wpx = pt[0];
  wpy = pt[1];
  wpz = pt[2];
  double distance = sqrt((ox - wpx) * (ox - wpx) + (oy - wpy) * (oy - wpy) + (oz - wpz) * (oz - wpz));
  double scaling_fact = fmax(fmin(1.0, (distance - 2 * g.res) / distance), 0.0);
  wpx = scaling_fact * (wpx - ox) + ox;
  wpy = scaling_fact * (wpy - oy) + oy;
  wpz = scaling_fact * (wpz - oz) + oz;
  double a = wpx - ox, bb = wpy - oy, c = wpz - oz, t = 1.0;
  if (wpz > cm.max_obstacle_height)
    t = fmax(0.0, fmin(t, (cm.max_obstacle_height - 0.01 - oz) / c));
  else if (wpz < cm.origin_z)
    t = fmin(t, (cm.origin_z - oz) / c);
  if (wpx < g.ox) t = fmin(t, (g.ox - ox) / a);
  if (wpy < g.oy) t = fmin(t, (g.oy - oy) / bb);
  if (wpx > r.map_end_x) t = fmin(t, (r.map_end_x - ox) / a);
  if (wpy > r.map_end_y) t = fmin(t, (r.map_end_y - oy) / bb);
  wpx = ox + a * t;
  wpy = oy + bb * t;
  wpz = oz + c * t;
  if (wpx < g.ox || wpy < g.oy || wpz < cm.origin_z) return false;
  px = (wpx - g.ox) / g.res;
  py = (wpy - g.oy) / g.res;
  pz = (wpz - cm.origin_z) / cm.z_resolution;
  return px < g.nx && py < g.ny && pz < size_z;
}

// navfn::NavFn arrays of a batch of plans (navfn_kernels.hip, navgpu_navfn.cpp)
struct NavfnDev {
  int nx, ny, ns;
  uint32_t ns_padded, path_cap;
  uint8_t *costarr, *pending;   // [n][ns_padded]
  float *potarr, *gradx, *grady;  // [n][ns_padded]
  int* pb;                      // [n][3][PRIORITYBUFSIZE]
  float* path;                  // [n][2][path_cap]: pathx, pathy
  navgpu_navfn_result* results; // [n]
  // tiled wavefront expansion (navgpu_navfn_plan_wavefront), allocated on first use
  float* potalt;                // [n][ns_padded] the second potential array (rounds alternate)
  uint32_t* wf_act;             // [n][2][tiles] marks of this / the next round: 1 copy across, 2 relax
  uint32_t *wf_nchg, *wf_min;   // [n][wf_max_rounds] tiles that changed in a round / smallest value it wrote (float bits)
  struct NavfnWfStatus* wf_status;  // [n]
  int wf_tiles_x, wf_tiles_y, wf_max_rounds;
};
struct NavfnWfStatus {
  int32_t done, final_array, rounds, pad;
};
// which update rule the tiled wavefront relaxes: NavFn::updateCell's (navfn.cpp:466-535) or DijkstraExpansion::updateCell's with
// its cost translation and either potential calculator (dijkstra.cpp:170-229, dijkstra.h:78-87)
struct NavfnWfRule {
  int32_t global_planner, quadratic, outline, allow_unknown;
  int32_t lethal_cost, neutral_cost;
  float cost_factor;
  int32_t max_sweeps;  // red / black sweeps of a tile per round
};
void launch_navfn_wf_init(const NavfnDev& nv, uint32_t first, uint32_t count, const NavfnWfRule& rule, const int32_t* seed_cells, const float* seed_vals,
                          hipStream_t s);
void launch_navfn_wf_round(const NavfnDev& nv, uint32_t first, uint32_t count, const NavfnWfRule& rule, const int32_t* stop_cells, int at_start, int round,
                           hipStream_t s);
void launch_gp_wf_finish(const NavfnDev& nv, uint32_t first, uint32_t count, const navgpu_global_planner_params& gp, const double* starts,
                         const double* goals, const int32_t* goal_cells, hipStream_t s);
void launch_navfn_wf_path(const NavfnDev& nv, uint32_t first, uint32_t count, const int32_t* goals, const int32_t* starts, hipStream_t s);
void launch_navfn_costmap(const NavfnDev& nv, uint32_t first, uint32_t count, const uint8_t* cmap, size_t stride, int cost_mode, int allow_unknown,
                          hipStream_t s);
void launch_gp_plan(const NavfnDev& nv, uint32_t first, uint32_t count, const navgpu_global_planner_params& gp, const double* starts,
                    const double* goals, const int32_t* goal_cells, void* heaps, hipStream_t s);
void launch_navfn_plan(const NavfnDev& nv, uint32_t first, uint32_t count, const int32_t* goals, const int32_t* starts, int astar, int at_start,
                       hipStream_t s);

}  // namespace navgpu
